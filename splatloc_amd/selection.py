"""Landmark selection of SplatLoc's test.py --eval_selection (utils/selection.py:91-157, gaussian_selectition) on the device.

The saliency score and the greedy spatial pick are the HIP of csrc/selection.hip behind the C ABI (include/splatraster.h,
splatraster_landmark_*).  `gaussian_selectition` is the drop-in for `from utils.selection import gaussian_selectition`
(INTEGRATION.md §16); `landmark_scores` and `select_landmarks` are the torch-level calls, on the current stream.  There is no
CPU fallback: without the device the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native
from ._host import _stream, device, ptr, workspace

WIDTH, HEIGHT = 640, 480   # the reference's inside_check hard-codes 640 x 480
RADIUS = 18.0


def _as(t, dtype, device) -> torch.Tensor:
    t = torch.as_tensor(t)
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _check_points(points: torch.Tensor):
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(points.shape)}")


def landmark_scores(points, w2cs, K, depths, width: int = WIDTH, height: int = HEIGHT) -> dict:
    """Per-point saliency of the reference's gaussian_selectition.  points [N,3], w2cs [M,4,4] world-to-camera, K [3,3],
    depths [M,>=height,>=width] (metres; the top-left height x width window is read).  Returns a dict of device tensors:
    n_visible, n_depth (int32), depth_mean, depth_std (NaN where no diff was kept), span, score (float64)."""
    points = torch.as_tensor(points)
    _check_points(points)
    w2cs = torch.as_tensor(w2cs)
    depths = torch.as_tensor(depths)
    if w2cs.dim() != 3 or tuple(w2cs.shape[1:]) != (4, 4):
        raise ValueError(f"w2cs must be [M, 4, 4], got {tuple(w2cs.shape)}")
    if depths.dim() != 3:
        raise ValueError(f"depths must be [M, H, W], got {tuple(depths.shape)}")
    if depths.shape[0] != w2cs.shape[0]:
        raise ValueError(f"{depths.shape[0]} depth maps for {w2cs.shape[0]} poses: each pose needs its own map")
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    if depths.shape[1] < height or depths.shape[2] < width:
        raise ValueError(f"depth maps are {depths.shape[1]} x {depths.shape[2]}, smaller than {height} x {width}")
    Kh = torch.as_tensor(K).detach().to("cpu", torch.float64).contiguous()
    if tuple(Kh.shape) != (3, 3):
        raise ValueError(f"K must be [3, 3], got {tuple(Kh.shape)}")
    dev = device("landmark selection")
    N, M = int(points.shape[0]), int(w2cs.shape[0])
    p = _as(points, torch.float32, dev)
    w = _as(w2cs, torch.float32, dev)
    d = _as(depths, torch.float32, dev)
    if d.shape[1] != height or d.shape[2] != width:
        d = d[:, :height, :width].contiguous()
    out = {"n_visible": torch.empty(N, dtype=torch.int32, device=dev),
           "n_depth": torch.empty(N, dtype=torch.int32, device=dev)}
    for k in ("depth_mean", "depth_std", "span", "score"):
        out[k] = torch.empty(N, dtype=torch.float64, device=dev)
    if N == 0:
        return out
    st = _native.load().splatraster_landmark_scores(
        N, M, ptr(p), ptr(w), C.cast(Kh.numpy().ctypes.data, C.c_void_p), ptr(d), width, height,
        ptr(out["n_visible"]), ptr(out["n_depth"]), ptr(out["depth_mean"]), ptr(out["depth_std"]), ptr(out["span"]),
        ptr(out["score"]), _stream(dev))
    _native.check(st, "splatraster_landmark_scores")
    return out


def select_landmarks(points, scores, num: int, radius: float = RADIUS, return_passes: bool = False):
    """The reference's greedy pick: indices [num] (int64, device) of the chosen points in pick order.  Candidates are
    walked by score descending; tied scores go the larger index first (a stable ascending sort, reversed).  Raises
    ValueError for num outside [1, N], non-finite points, or fewer than num distinct positions."""
    points = torch.as_tensor(points)
    _check_points(points)
    scores = torch.as_tensor(scores)
    N = int(points.shape[0])
    if scores.dim() != 1 or scores.shape[0] != N:
        raise ValueError(f"scores must be [{N}], got {tuple(scores.shape)}")
    num = int(num)
    if num < 1 or num > N:
        raise ValueError(f"num must be in [1, {N}] (the number of points), got {num}")
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    dev = device("landmark selection")
    p = _as(points, torch.float32, dev)
    s = _as(scores, torch.float64, dev)
    if not bool(torch.isfinite(p).all()):
        raise ValueError("points must be finite")
    distinct = torch.unique(p, dim=0).shape[0] if num > 1 else 1
    if distinct < num:
        raise ValueError(f"only {distinct} distinct positions for {num} landmarks: the reference would halve the radius to 0 "
                         "and repeat points")
    lib = _native.load()
    ws = workspace(lib.splatraster_landmark_workspace_bytes(N, num), dev)
    out = torch.empty(num, dtype=torch.int32, device=dev)
    passes = C.c_int32(0)
    st = lib.splatraster_landmark_select(N, C.c_void_p(p.data_ptr()), C.c_void_p(s.data_ptr()), num, radius,
                                         C.c_void_p(out.data_ptr()), C.byref(passes), C.c_void_p(ws.data_ptr()),
                                         _stream(dev))
    _native.check(st, "splatraster_landmark_select")
    idx = out.long()
    return (idx, int(passes.value)) if return_passes else idx


def gaussian_selectition(points3D, wc2s, intrinsics, depths, num_gs=100):
    """Drop-in for utils/selection.py's gaussian_selectition (its name and signature): the num_gs chosen points [num_gs, 3]
    as numpy float64, in pick order.  Deviations from the reference are listed in INTEGRATION.md §16."""
    pts = torch.as_tensor(points3D)
    _check_points(pts)
    N = int(pts.shape[0])
    num_gs = int(num_gs)
    if num_gs < 1 or num_gs > N:
        raise ValueError(f"num_gs must be in [1, {N}] (the number of points), got {num_gs}")
    sc = landmark_scores(pts, wc2s, intrinsics, depths)
    idx = select_landmarks(pts, sc["score"], num_gs)
    return pts.detach().to(device=idx.device, dtype=torch.float32)[idx].cpu().numpy().astype(np.float64)


gaussian_selection = gaussian_selectition
