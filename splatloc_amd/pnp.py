"""Absolute pose of SplatLoc's test.py --eval_pose (solve_pose, test.py:64-84) on the device.

P3P LO-RANSAC and the Cauchy-loss refinement are the HIP of csrc/pnp.hip behind the C ABI (include/splatraster.h,
splatraster_pnp*).  `absolute_pose_estimation` has the signature and result dict of the pycolmap call solve_pose was written
against, `solve_pose` is the drop-in for test.py's function, `estimate_absolute_pose(_batch)` keep everything on the device
(INTEGRATION.md §18).  There is no CPU fallback: without the device the calls raise.  Argument checks run before any device
work.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native
from ._host import _stream, device, float_tensor, workspace
from ._host import ptr as _ptr   # tests call pnp._ptr

MAX_N = 1 << 20          # SPLATRASTER_PNP_MAX_N
BATCH = 1024             # SPLATRASTER_PNP_BATCH: trials per round trip
PNP_OK, PNP_NO_MODEL, PNP_NONFINITE = 0, 1, 2
CAMERA_MODELS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "OPENCV": 8}
DEFAULTS = dict(max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, confidence=0.9999,
                seed=0)


class PnpProblem(C.Structure):
    """struct splatraster_pnp_problem"""
    _fields_ = [("offset", C.c_int64), ("n", C.c_int32), ("reserved", C.c_int32), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class PnpOptions(C.Structure):
    """struct splatraster_pnp_options"""
    _fields_ = [("max_error_px", C.c_double), ("min_inlier_ratio", C.c_double), ("confidence", C.c_double),
                ("seed", C.c_uint64), ("min_num_trials", C.c_int32), ("max_num_trials", C.c_int32)]


def options(max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, confidence=0.9999, seed=0):
    """checked PnpOptions (ValueError for a bad value)"""
    max_error_px, min_inlier_ratio, confidence = float(max_error_px), float(min_inlier_ratio), float(confidence)
    if not (max_error_px > 0) or not math.isfinite(max_error_px):
        raise ValueError(f"max_error_px must be positive and finite, got {max_error_px}")
    if not (0.0 < confidence < 1.0):
        raise ValueError(f"confidence must lie in (0, 1), got {confidence}")
    if not (0.0 <= min_inlier_ratio <= 1.0):
        raise ValueError(f"min_inlier_ratio must lie in [0, 1], got {min_inlier_ratio}")
    min_num_trials, max_num_trials = int(min_num_trials), int(max_num_trials)
    if min_num_trials < 1 or max_num_trials >= 1 << 31:
        raise ValueError(f"trial limits must lie in [1, 2^31), got {min_num_trials} and {max_num_trials}")
    if min_num_trials > max_num_trials:
        raise ValueError(f"min_num_trials ({min_num_trials}) > max_num_trials ({max_num_trials})")
    return PnpOptions(max_error_px, min_inlier_ratio, confidence, int(seed) & ((1 << 64) - 1), min_num_trials, max_num_trials)


def camera_intrinsics(camera):
    """(fx, fy, cx, cy) of a pycolmap-style camera dict {"model", "width", "height", "params"}"""
    if not isinstance(camera, dict) or "model" not in camera or "params" not in camera:
        raise ValueError("camera must be a dict with 'model', 'width', 'height' and 'params'")
    model = str(camera["model"])
    if model not in CAMERA_MODELS:
        raise ValueError(f"unsupported camera model {model!r}: SIMPLE_PINHOLE, PINHOLE or OPENCV without distortion")
    p = [float(x) for x in np.asarray(camera["params"], dtype=np.float64).reshape(-1)]
    if len(p) != CAMERA_MODELS[model]:
        raise ValueError(f"{model} takes {CAMERA_MODELS[model]} params, got {len(p)}")
    if not all(math.isfinite(x) for x in p):
        raise ValueError("camera params must be finite")
    if model == "SIMPLE_PINHOLE":
        fx = fy = p[0]
        cx, cy = p[1], p[2]
    else:
        fx, fy, cx, cy = p[:4]
        if model == "OPENCV" and any(x != 0.0 for x in p[4:]):
            raise ValueError("OPENCV distortion must be zero: distortion models are not supported")
    if fx == 0.0 or fy == 0.0:
        raise ValueError("focal lengths must be nonzero")
    return fx, fy, cx, cy


def _K_intrinsics(K):
    k = torch.as_tensor(K).detach().to("cpu", torch.float64)
    if tuple(k.shape) != (3, 3):
        raise ValueError(f"K must be [3, 3], got {tuple(k.shape)}")
    if not bool(torch.isfinite(k).all()):
        raise ValueError("K must be finite")
    if k[0, 1] != 0 or k[1, 0] != 0 or k[2, 0] != 0 or k[2, 1] != 0 or k[2, 2] != 1:
        raise ValueError("K must be a pinhole matrix [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
    fx, fy, cx, cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if fx == 0.0 or fy == 0.0:
        raise ValueError("focal lengths must be nonzero")
    return fx, fy, cx, cy


def _points(p2d, p3d):
    """checked (points2D [N, 2], points3D [N, 3]) tensors, not yet moved or widened"""
    a, b = float_tensor(p2d, "points2D"), float_tensor(p3d, "points3D")
    if a.dim() != 2 or a.shape[1] != 2:
        raise ValueError(f"points2D must be [N, 2], got {tuple(a.shape)}")
    if b.dim() != 2 or b.shape[1] != 3:
        raise ValueError(f"points3D must be [N, 3], got {tuple(b.shape)}")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"points2D and points3D differ in length: {a.shape[0]} and {b.shape[0]}")
    if a.shape[0] > MAX_N:
        raise ValueError(f"{a.shape[0]} correspondences: at most 2^20 are supported")
    if not (bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())):
        raise ValueError("points2D and points3D must be finite")
    return a, b


def _solve(items, opt, dev):
    """one splatraster_pnp call over items [(p2d, p3d, (fx, fy, cx, cy))] (checked); device tensors per problem"""
    lib = _native.load()
    B = len(items)
    table, off = [], 0
    for a, _, (fx, fy, cx, cy) in items:
        table.append(PnpProblem(off, int(a.shape[0]), 0, fx, fy, cx, cy))
        off += int(a.shape[0])
    tab = (PnpProblem * B)(*table)
    p2 = torch.cat([a.detach().to(device=dev, dtype=torch.float64).reshape(-1, 2) for a, _, _ in items]).contiguous()
    p3 = torch.cat([b.detach().to(device=dev, dtype=torch.float64).reshape(-1, 3) for _, b, _ in items]).contiguous()
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    ninl = torch.empty(B, dtype=torch.int32, device=dev)
    mask = torch.empty(max(off, 1), dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    trials = torch.empty(B, dtype=torch.int32, device=dev)
    ws = workspace(lib.splatraster_pnp_workspace_bytes(B, tab, C.byref(opt)), dev)
    st = lib.splatraster_pnp(B, tab, C.byref(opt), _ptr(p2), _ptr(p3), _ptr(R), _ptr(t), _ptr(ninl), _ptr(mask), _ptr(status),
                             _ptr(trials), _ptr(ws), _stream(dev))
    _native.check(st, "splatraster_pnp")
    out = []
    for b, tb in enumerate(table):
        out.append({"R": R[b], "t": t[b], "inliers": mask[tb.offset:tb.offset + tb.n].bool(), "num_inliers": ninl[b],
                    "success": status[b] == PNP_OK, "trials": trials[b]})
    return out


def estimate_absolute_pose(p2d, p3d, K, max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000,
                           max_num_trials=100000, confidence=0.9999, seed=0):
    """P3P LO-RANSAC + refinement on the device.  p2d [N, 2] pixels, p3d [N, 3] world points, K [3, 3] pinhole.  Returns device
    tensors {R [3, 3] f64, t [3] f64 (world-to-camera), inliers bool [N], num_inliers, success, trials}; N < 4 gives
    success False without a launch."""
    return estimate_absolute_pose_batch([(p2d, p3d, K)], max_error_px, min_inlier_ratio, min_num_trials, max_num_trials,
                                        confidence, seed)[0]


def estimate_absolute_pose_batch(problems, max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000,
                                 max_num_trials=100000, confidence=0.9999, seed=0):
    """estimate_absolute_pose of every (p2d, p3d, K) of `problems` in one launch sequence: a list of result dicts, each
    bit-identical to the single-problem call."""
    opt = options(max_error_px, min_inlier_ratio, min_num_trials, max_num_trials, confidence, seed)
    items = []
    for p in problems:
        if len(p) != 3:
            raise ValueError("a problem is (p2d, p3d, K)")
        a, b = _points(p[0], p[1])
        items.append((a, b, _K_intrinsics(p[2])))
    if len(items) > 65535:
        raise ValueError("at most 65535 problems per batch")
    dev = device("absolute pose estimation")
    run = [i for i, (a, _, _) in enumerate(items) if a.shape[0] >= 4]
    solved = _solve([items[i] for i in run], opt, dev) if run else []
    out = [None] * len(items)
    for i, r in zip(run, solved):
        out[i] = r
    for i, (a, _, _) in enumerate(items):
        if out[i] is None:
            out[i] = {"R": torch.zeros((3, 3), dtype=torch.float64, device=dev),
                      "t": torch.zeros(3, dtype=torch.float64, device=dev),
                      "inliers": torch.zeros(a.shape[0], dtype=torch.bool, device=dev),
                      "num_inliers": torch.zeros((), dtype=torch.int32, device=dev),
                      "success": torch.zeros((), dtype=torch.bool, device=dev),
                      "trials": torch.zeros((), dtype=torch.int32, device=dev)}
    return out


def rotmat_to_qvec(R):
    """unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (Shepperd's method)"""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * math.sqrt(tr + 1.0)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = 2.0 * math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def qvec_to_rotmat(q):
    """rotation matrix of a quaternion (w, x, y, z), normalised first"""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _absolute_pose(points2D, points3D, camera, **kw):
    """(result dict, refined world-to-camera rotation matrix or None)"""
    opt_kw = {k: kw.get(k, v) for k, v in DEFAULTS.items()}
    options(**opt_kw)
    a, b = _points(points2D, points3D)
    intr = camera_intrinsics(camera)
    if a.shape[0] < 4:
        return {"success": False}, None
    r = _solve([(a, b, intr)], options(**opt_kw), device("absolute pose estimation"))[0]
    if not bool(r["success"].cpu()):
        return {"success": False}, None
    R = r["R"].cpu().numpy()
    t = r["t"].cpu().numpy()
    return {"success": True, "qvec": rotmat_to_qvec(R), "tvec": t, "num_inliers": int(r["num_inliers"].cpu()),
            "inliers": r["inliers"].cpu().numpy()}, R


def absolute_pose_estimation(points2D, points3D, camera, max_error_px=12.0, min_inlier_ratio=0.01, min_num_trials=1000,
                             max_num_trials=100000, confidence=0.9999, seed=0):
    """pycolmap.absolute_pose_estimation as solve_pose calls it: {"success": False} on failure, else {"success": True,
    "qvec" (w, x, y, z; unit, w >= 0), "tvec", "num_inliers", "inliers" (numpy bool [N])} with x_cam = R(qvec) X + tvec.
    camera: {"model": SIMPLE_PINHOLE | PINHOLE | OPENCV (zero distortion), "width", "height", "params"}."""
    return _absolute_pose(points2D, points3D, camera, max_error_px=max_error_px, min_inlier_ratio=min_inlier_ratio,
                          min_num_trials=min_num_trials, max_num_trials=max_num_trials, confidence=confidence, seed=seed)[0]


def solve_pose(kp_2d, kp_3d, intrinsics):
    """Drop-in for test.py's solve_pose: (R_c2w, t_c2w, ret) on success, (None, None, ret) on failure.  The camera-to-world
    pose is taken from the refined rotation matrix: R_c2w = R^T, t_c2w = -R^T t."""
    ret, R = _absolute_pose(kp_2d, kp_3d, intrinsics)
    if not ret["success"]:
        return None, None, ret
    rmatrix = np.transpose(R)
    t = -rmatrix @ np.asarray(ret["tvec"], dtype=np.float64)
    return rmatrix, t, ret
