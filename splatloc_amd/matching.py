"""2D-3D matching of SplatLoc's test.py --eval_pose (LocalizeQuery.match_feature, test.py:247-378) on the device.

The exact assignment solver, the descriptor cost matrix and the frustum candidates are the HIP of csrc/matching.hip behind the
C ABI (include/splatraster.h, splatraster_lsap*, splatraster_match_*, splatraster_frustum_*).  `hungarian_solve` and
`HungarianMatcher` are the drop-ins for `utils/match_utils.py`, `get_frusm_pts` restates the method of the same name
(INTEGRATION.md §17).  `linear_sum_assignment` returns scipy's assignment exactly, ties included.  There is no CPU fallback:
without the device the calls raise.  Argument checks that need no data run before any device work.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native
from ._host import _stream, device, float_tensor, workspace
from ._host import ptr as _ptr   # tests and tools call matching._ptr

MAX_NC = 65535          # SPLATRASTER_LSAP_MAX_NC: the solver's 16-bit column indices
MAX_ELEMENTS = 1 << 31  # nr * nc must stay below
LSAP_OK, LSAP_INVALID, LSAP_INFEASIBLE = 0, 1, 2
THRESHOLD = 0.4         # hungarian_solve's similarity floor
SP_KP_THRE = 0.005      # LocalizeQuery.sp_kp_thre (test.py:107)
NN_RADIUS = 0.1         # get_frusm_pts' distance_upper_bound


class LsapProblem(C.Structure):
    """struct splatraster_lsap_problem"""
    _fields_ = [("offset", C.c_int64), ("nr", C.c_int32), ("nc", C.c_int32), ("transposed", C.c_int32),
                ("reserved", C.c_int32)]


def _check_cost(cost):
    shape = tuple(cost.shape) if hasattr(cost, "shape") else np.shape(cost)
    if len(shape) != 2:
        raise ValueError(f"expected a matrix (2-D array), got a {len(shape)} array")
    nr, nc = int(shape[0]), int(shape[1])
    lo, hi = min(nr, nc), max(nr, nc)
    if hi > MAX_NC:
        raise ValueError(f"cost matrix is {nr} x {nc}: the device solver takes at most {MAX_NC} columns after orientation "
                         "(the larger dimension)")
    if lo * hi >= MAX_ELEMENTS:
        raise ValueError(f"cost matrix is {nr} x {nc}: the device solver takes fewer than 2^31 entries")
    return float_tensor(cost, "cost matrix")


def _lsap_launch(costs, problems, B, maximize, dev, total):
    """one splatraster_lsap call, no host read: (rows, cols, status, steps) device tensors"""
    lib = _native.load()
    table = (LsapProblem * max(B, 1))(*problems)
    rows = torch.empty(total, dtype=torch.int64, device=dev)
    cols = torch.empty(total, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    steps = torch.empty(B, dtype=torch.int32, device=dev)
    ws = workspace(lib.splatraster_lsap_workspace_bytes(B, table), dev)
    st = lib.splatraster_lsap(B, table, _ptr(costs), 1 if maximize else 0, _ptr(rows), _ptr(cols), _ptr(status), _ptr(steps),
                              _ptr(ws), _stream(dev))
    _native.check(st, "splatraster_lsap")
    return rows, cols, status, steps


def _lsap_raise(status_host):
    """scipy's ValueError messages for a host copy of the solver's status words"""
    if bool((status_host == LSAP_INVALID).any()):
        raise ValueError("matrix contains invalid numeric entries")
    if bool((status_host == LSAP_INFEASIBLE).any()):
        raise ValueError("cost matrix is infeasible")


def _solve(costs, problems, B, maximize, dev, total):
    """one splatraster_lsap call; returns (rows, cols, steps) device tensors, raises scipy's ValueError messages"""
    rows, cols, status, steps = _lsap_launch(costs, problems, B, maximize, dev, total)
    _lsap_raise(status.cpu())   # the one host read of the call
    return rows, cols, steps


def _cost_launch(a, b, threshold, norms, cost, offset, dev):
    """splatraster_match_cost of a [D, N1], b [D, N2] (f32, device) into the N1 * N2 entries of `cost` (f64) from element
    `offset`; norms [N1 + N2] is written too"""
    st = _native.load().splatraster_match_cost(int(a.shape[0]), int(a.shape[1]), int(b.shape[1]), _ptr(a), _ptr(b),
                                               float(threshold), _ptr(norms), C.c_void_p(cost.data_ptr() + 8 * offset),
                                               _stream(dev))
    _native.check(st, "splatraster_match_cost")


def _orient(t, dev):
    """f64 device copy in the solver's orientation (rows <= columns) and whether it was transposed"""
    t = t.to(device=dev, dtype=torch.float64)
    tr = t.shape[1] < t.shape[0]
    return (t.t() if tr else t).contiguous().reshape(-1), tr


def linear_sum_assignment(cost, maximize=False, return_steps=False):
    """scipy.optimize.linear_sum_assignment on the device: (row_ind, col_ind) int64 device tensors, scipy's assignment exactly.
    cost: numpy or torch float32 / float64 [nr, nc] (float32 is widened exactly, as scipy does).  Raises scipy's ValueError
    for NaN / -inf entries ("matrix contains invalid numeric entries") and for "cost matrix is infeasible"."""
    t = _check_cost(cost)
    dev = device("2D-3D matching")
    nr, nc = int(t.shape[0]), int(t.shape[1])
    if nr == 0 or nc == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return (e, e.clone(), 0) if return_steps else (e, e.clone())
    flat, tr = _orient(t, dev)
    p = LsapProblem(0, min(nr, nc), max(nr, nc), int(tr), 0)
    rows, cols, steps = _solve(flat, [p], 1, maximize, dev, min(nr, nc))
    return (rows, cols, int(steps.cpu()[0])) if return_steps else (rows, cols)


def linear_sum_assignment_batch(costs, maximize=False, return_steps=False):
    """linear_sum_assignment of every matrix of `costs` (a sequence of differently shaped matrices) in one launch: a list of
    (row_ind, col_ind).  One host read for the whole batch; an invalid or infeasible member raises for the batch."""
    ts = [_check_cost(c) for c in costs]
    dev = device("2D-3D matching")
    pieces, problems, shapes, off, total = [], [], [], 0, 0
    for t in ts:
        nr, nc = int(t.shape[0]), int(t.shape[1])
        shapes.append(min(nr, nc))
        if nr == 0 or nc == 0:
            continue
        flat, tr = _orient(t, dev)
        pieces.append(flat)
        problems.append(LsapProblem(off, min(nr, nc), max(nr, nc), int(tr), 0))
        off += flat.numel()
        total += min(nr, nc)
    if problems:
        rows, cols, steps = _solve(torch.cat(pieces), problems, len(problems), maximize, dev, total)
    else:
        rows = cols = torch.empty(0, dtype=torch.int64, device=dev)
        steps = torch.empty(0, dtype=torch.int32)
    out, o = [], 0
    for k in shapes:
        out.append((rows[o:o + k], cols[o:o + k]))
        o += k
    if return_steps:
        return out, [int(s) for s in steps.cpu()]
    return out


def _check_descriptors(d1, d2):
    a = float_tensor(d1, "descriptors1")
    b = float_tensor(d2, "descriptors2")
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"descriptors must be [D, N], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"descriptor dimensions differ: {a.shape[0]} and {b.shape[0]}")
    if a.shape[0] < 1:
        raise ValueError("descriptors must have at least one dimension")
    n1, n2 = int(a.shape[1]), int(b.shape[1])
    if n1 and n2 and (max(n1, n2) > MAX_NC or n1 * n2 >= MAX_ELEMENTS):
        raise ValueError(f"{n1} x {n2} descriptors: the device solver takes at most {MAX_NC} of the larger set and fewer than "
                         "2^31 pairs")
    return a, b


def match_descriptors(d1, d2, threshold=THRESHOLD, return_steps=False):
    """hungarian_solve on the device: d1 [D, N1], d2 [D, N2] (columns are descriptors).  Returns device tensors
    matches [2, min(N1, N2)] (int64: d1 index, d2 index, ascending by d1 index) and sims [min(N1, N2)] (f32, the thresholded
    similarity of each pair, 0 for the pairs below threshold the assignment still makes)."""
    a, b = _check_descriptors(d1, d2)
    dev = device("2D-3D matching")
    D, N1, N2 = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if N1 == 0 or N2 == 0:
        m = torch.empty((2, 0), dtype=torch.int64, device=dev)
        s = torch.empty(0, dtype=torch.float32, device=dev)
        return (m, s, 0) if return_steps else (m, s)
    a = a.detach().to(device=dev, dtype=torch.float32).contiguous()
    b = b.detach().to(device=dev, dtype=torch.float32).contiguous()
    norms = torch.empty(N1 + N2, dtype=torch.float32, device=dev)
    cost = torch.empty(N1 * N2, dtype=torch.float64, device=dev)
    _cost_launch(a, b, threshold, norms, cost, 0, dev)
    K = min(N1, N2)
    p = LsapProblem(0, K, max(N1, N2), int(N2 < N1), 0)
    rows, cols, steps = _solve(cost, [p], 1, False, dev, K)
    sims = torch.empty(K, dtype=torch.float32, device=dev)
    _native.check(_native.load().splatraster_match_sims(D, N1, N2, _ptr(a), _ptr(b), _ptr(norms), float(threshold), K, _ptr(rows),
                                                        _ptr(cols), _ptr(sims), _stream(dev)), "splatraster_match_sims")
    m = torch.stack([rows, cols], dim=0)
    return (m, sims, int(steps.cpu()[0])) if return_steps else (m, sims)


def hungarian_solve(descriptors1, descriptors2):
    """Drop-in for utils/match_utils.py's hungarian_solve: (matches [2, min(N1, N2)] CPU int64, sims CPU float32).
    Deviations (empty inputs, mismatched dimensions, f32 summation order) are listed in INTEGRATION.md §17."""
    m, s = match_descriptors(descriptors1, descriptors2)
    return m.cpu(), s.cpu()


class HungarianMatcher:
    """Drop-in for utils/match_utils.py's HungarianMatcher."""

    def __init__(self):
        pass

    def __call__(self, data):
        for key in ("query_descs", "train_descs"):
            if key not in data:
                raise ValueError(key + " not exist in input")
        matches, scores = hungarian_solve(data["query_descs"], data["train_descs"])
        return {"matches": matches, "scores": scores}


def _host_f64(a, shape, what):
    t = torch.as_tensor(a).detach().to("cpu", torch.float64).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must be {list(shape)}, got {tuple(t.shape)}")
    return t


def frustum_candidates(points, w2c, K, width, height, marker=None, kp_mask=None, depth=None, c2w=None, kp_K=None,
                       marker_threshold=SP_KP_THRE):
    """get_frusm_pts' candidate stage on the device.  points [N,3] (f32), w2c [4,4] world-to-camera, K [3,3].
    Subset mode (marker None): the points inside the frustum (pc.z > 0.05, 0 <= u < width, 0 <= v < height) in index order.
    Key-Gaussian mode: also marker > marker_threshold; then every pixel of kp_mask == 1 ([height, width], row-major order) is
    back-projected with depth [height, width], c2w [4,4] and kp_K [3,3] and paired with its nearest kept point when closer
    than 0.1 (ties: the smaller index).  Returns device tensors (idx int64 [n], xyz f32 [n,3], uv f64 [n,2])."""
    pts = float_tensor(points, "points")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(pts.shape)}")
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    N = int(pts.shape[0])
    if N >= (1 << 31) - 1 or width * height >= (1 << 31) - 1:
        raise ValueError("frustum_candidates takes fewer than 2^31 - 1 points and pixels")
    w2c_h = _host_f64(w2c, (4, 4), "w2c")
    K_h = _host_f64(K, (3, 3), "K")
    key = marker is not None
    if key:
        mk = torch.as_tensor(marker).reshape(-1)
        if mk.shape[0] != N:
            raise ValueError(f"marker must hold {N} values, got {mk.shape[0]}")
        if kp_mask is None or depth is None or c2w is None or kp_K is None:
            raise ValueError("key-Gaussian mode needs kp_mask, depth, c2w and kp_K")
        km = torch.as_tensor(kp_mask)
        dp = torch.as_tensor(depth)
        if tuple(km.shape) != (height, width) or tuple(dp.shape) != (height, width):
            raise ValueError(f"kp_mask and depth must be [{height}, {width}], got {tuple(km.shape)} and {tuple(dp.shape)}")
        c2w_h = _host_f64(c2w, (4, 4), "c2w")
        kK = _host_f64(kp_K, (3, 3), "kp_K")
        kp4 = torch.tensor([kK[0, 0], kK[1, 1], kK[0, 2], kK[1, 2]], dtype=torch.float64)
    dev = device("2D-3D matching")
    p = pts.detach().to(device=dev, dtype=torch.float32).contiguous()
    cap = width * height if key else N
    idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    xyz = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
    uv = torch.empty((max(cap, 1), 2), dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = _native.load()
    ws = workspace(lib.splatraster_frustum_workspace_bytes(N, width, height), dev)
    hp = lambda t: C.cast(t.numpy().ctypes.data, C.c_void_p)  # noqa: E731
    if key:
        m = mk.detach().to(device=dev, dtype=torch.float32).contiguous()
        kmd = (km.to(dev) == 1).to(torch.uint8).contiguous()
        dd = dp.detach().to(device=dev, dtype=torch.float32).contiguous()
        st = lib.splatraster_frustum_candidates(N, _ptr(p), _ptr(m), float(marker_threshold), hp(w2c_h), hp(K_h), width, height,
                                                _ptr(kmd), _ptr(dd), hp(c2w_h), hp(kp4), _ptr(idx), _ptr(xyz), _ptr(uv),
                                                _ptr(count), _ptr(ws), _stream(dev))
    else:
        st = lib.splatraster_frustum_candidates(N, _ptr(p), None, float(marker_threshold), hp(w2c_h), hp(K_h), width, height,
                                                None, None, None, None, _ptr(idx), _ptr(xyz), _ptr(uv), _ptr(count), _ptr(ws),
                                                _stream(dev))
    _native.check(st, "splatraster_frustum_candidates")
    n = int(count.cpu()[0])   # the one host read of the call
    return idx[:n].long(), xyz[:n], uv[:n]


def get_frusm_pts(points, marker, frame, K, width, height, decoder, subset=None):
    """LocalizeQuery.get_frusm_pts (test.py:247-285) on the device: (ref_pts_3d numpy [n,3] (f32; subset mode: subset's dtype), decoder(torch.from_numpy(
    ref_pts_3d)), ref_pts_2d f64 numpy [n,2]).  points / marker: the key Gaussians' xyz and marker (gaussians.get_xyz,
    get_marker); frame: the dataset frame (w2c, c2w, K, depth, sp_kp_mask); K / width / height: the training dataset's
    intrinsics and size.  subset (the --eval_selection landmarks [M,3]) switches to frustum culling only."""
    if subset is not None:
        idx, xyz, uv = frustum_candidates(subset, frame["w2c"], K, width, height)
    else:
        idx, xyz, uv = frustum_candidates(points, frame["w2c"], K, width, height, marker=marker, kp_mask=frame["sp_kp_mask"],
                                          depth=frame["depth"], c2w=frame["c2w"], kp_K=frame["K"])
    if subset is not None:   # the reference indexes subset_xyz itself (float64 from gaussian_selectition)
        ref_pts_3d = np.asarray(subset.cpu() if torch.is_tensor(subset) else subset)[idx.cpu().numpy()]
    else:
        ref_pts_3d = xyz.cpu().numpy()
    ref_pts_2d = uv.cpu().numpy()
    ref_feats_3d = decoder(torch.from_numpy(ref_pts_3d))
    return ref_pts_3d, ref_feats_3d, ref_pts_2d
