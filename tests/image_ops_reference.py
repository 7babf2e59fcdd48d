"""The frame-preparation stage restated in numpy (include/splatraster.h "frame preparation"; utils/utils.py:4-38, 85-96 and
utils/camera_utils.py:145-172 of the reference): seeded case builders, the model in float32 in the kernel's stated summation order
(bit for bit what csrc/image_ops.hip computes) and in float64 (the oracle the reference's own float32 error is measured against),
the wrong models the tests must tell from the right one, and the bounds.

Bounds follow tests/loss_reference.py: MARGIN times the reference's own float32 error against the float64 oracle, taken from the
fixture tests/golden/image_ops.npz (never from the code under test), floored at one float32 ulp of the map's largest element.  A 0 / 1
decision x > t may differ from the fixture only where the oracle puts x within that bound times (1 + edge_threshold) of t: x moves by
the bound, t = median * edge_threshold by edge_threshold times the bound.
"""
import hashlib

import numpy as np

MARGIN = 4.0
EPS32 = float(np.finfo(np.float32).eps)
BLOCKS = 32
EPS = 0.01
WV = (3.0, 10.0, 3.0, 0.0, 0.0, 0.0, -3.0, -10.0, -3.0)
WH = (3.0, 0.0, -3.0, 10.0, 0.0, -10.0, 3.0, 0.0, -3.0)
NEAR_MAX_FRACTION = 0.001    # pixels of a case a test may excuse as too near the threshold


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest()[:16], dtype=np.uint8).copy()


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def map_bound(ref32, oracle64):
    """MARGIN * max |ref32 - oracle64| over the finite elements, floored at one float32 ulp of the map's largest element"""
    o = np.asarray(oracle64, np.float64)
    r = np.asarray(ref32, np.float64).reshape(o.shape)
    ok = np.isfinite(o) & np.isfinite(r)
    if not ok.any():
        return ulp32(1.0)
    return max(MARGIN * float(np.abs(r[ok] - o[ok]).max()), ulp32(np.abs(o[ok]).max()))


# =================================================================================================================================
# cases
# =================================================================================================================================
# name: H, W, dataset type, edge_threshold, intensity scale, seed, NaN pixel (y, x) or None, in the fixture, what it pins
CASES = {
    "replica_32x32": dict(H=32, W=32, type="replica", thr=4.0, scale=1.0, seed=11, nan=None, golden=True, path="lds_small"),     # n = 1
    "replica_64x96": dict(H=64, W=96, type="replica", thr=4.0, scale=1.0, seed=12, nan=None, golden=True, path="lds_small"),     # n = 6: even
    "replica_96x96": dict(H=96, W=96, type="replica", thr=4.0, scale=1.0, seed=13, nan=None, golden=True, path="lds_small"),     # n = 9: odd
    "replica_75x110": dict(H=75, W=110, type="replica", thr=4.0, scale=1.0, seed=14, nan=None, golden=True, path="lds_small"),   # remainder
    "scenes12_75x110": dict(H=75, W=110, type="12scenes", thr=4.0, scale=1.0, seed=14, nan=None, golden=True, path="lds_small"),
    "replica_255_64x96": dict(H=64, W=96, type="replica", thr=1.0, scale=255.0, seed=15, nan=None, golden=True, path="lds_small"),   # t >= 1
    "replica_nan_64x96": dict(H=64, W=96, type="replica", thr=4.0, scale=1.0, seed=16, nan=(33, 50), golden=True, path="lds_small"),
    "scenes12_nan_64x96": dict(H=64, W=96, type="12scenes", thr=4.0, scale=1.0, seed=16, nan=(33, 50), golden=True, path="lds_small"),
    "replica_640x640": dict(H=640, W=640, type="replica", thr=4.0, scale=1.0, seed=17, nan=None, golden="packed", path="lds_small"),   # n = 400
    # the boundary between the fused kernel and the per-block select over global memory; too large for a fixture
    "replica_4096x4096": dict(H=4096, W=4096, type="replica", thr=4.0, scale=1.0, seed=18, nan=None, golden=False, path="lds_big", tile=8),   # n = 16 384
    "replica_3616x4640": dict(H=3616, W=4640, type="replica", thr=4.0, scale=1.0, seed=19, nan=None, golden=False, path="global", tile=8),   # n = 16 385
}
SMALL_CASES = tuple(k for k, c in CASES.items() if c["golden"] is True)
GOLDEN_CASES = tuple(k for k, c in CASES.items() if c["golden"])


def frame(H, W, seed, scale=1.0, nan=None):
    """A structured frame [3,H,W] float32: a smooth product of sinusoids per channel, a bright rectangle, 2 % noise, clipped to 0..1,
    a zeroed corner (so that validity matters), times `scale`; optionally one NaN pixel in channel 1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((3, H, W), np.float64)
    for c in range(3):
        fx, fy = rng.uniform(1.5, 4.5, 2)
        px, py = rng.uniform(0, 2 * np.pi, 2)
        img[c] = 0.45 + 0.35 * np.sin(2 * np.pi * fx * x / W + px) * np.sin(2 * np.pi * fy * y / H + py)
    img[:, H // 4:H // 2, W // 3:2 * W // 3] += 0.3
    img += 0.02 * rng.standard_normal((3, H, W))
    img = np.clip(img, 0.0, 1.0)
    img[:, :max(H // 5, 3), :max(W // 6, 3)] = 0.0
    img = (img * scale).astype(np.float32)
    if nan is not None:
        img[1, nan[0], nan[1]] = np.nan
    return img


def case_image(name):
    """the case's frame; the two large cases tile a frame of an eighth of their size plus (3, 5) pixels (cheap to build; the period is no
    multiple of the block, so every block differs)"""
    c = CASES[name]
    t = c.get("tile")
    if not t:
        return frame(c["H"], c["W"], c["seed"], c["scale"], c["nan"])
    base = frame(c["H"] // t + 3, c["W"] // t + 5, c["seed"], c["scale"], c["nan"])
    return np.ascontiguousarray(np.tile(base, (1, t, t))[:, :c["H"], :c["W"]])


# =================================================================================================================================
# the model
# =================================================================================================================================
def gray_of(img, dt):
    img = np.asarray(img, dt)
    return ((img[0] + img[1]) + img[2]) / dt(3)


def gradients(plane, dt, pad="reflect"):
    """grad_v, grad_h of one plane: cross-correlation with the Scharr kernels over 32, the nine products added row-major"""
    H, W = plane.shape
    with np.errstate(invalid="ignore"):
        p = np.pad(np.asarray(plane, dt), 1, mode=pad)
        taps = [p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
        av, ah = dt(WV[0]) * taps[0], dt(WH[0]) * taps[0]
        for k in range(1, 9):
            av = av + dt(WV[k]) * taps[k]
            ah = ah + dt(WH[k]) * taps[k]
        return dt(0.03125) * av, dt(0.03125) * ah


def validity(plane, dt, eps=EPS, pad="reflect", centre_only=False):
    H, W = plane.shape
    with np.errstate(invalid="ignore"):
        ok = np.abs(np.pad(np.asarray(plane, dt), 1, mode=pad)) > dt(np.float32(eps))
    if centre_only:
        return ok[1:1 + H, 1:1 + W]
    out = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out &= ok[dy:dy + H, dx:dx + W]
    return out


def intensity_of(gv, gh, valid, dt):
    with np.errstate(invalid="ignore"):
        m = valid.astype(dt)
        a, b = gv * m, gh * m
        return np.sqrt(a * a + b * b)


def lower_median(v, upper=False):
    """element (n - 1) / 2 of the ascending order (n / 2: the wrong, upper one); NaN when any element is NaN"""
    v = np.asarray(v).ravel()
    if np.isnan(v).any():
        return v.dtype.type(np.nan)
    return np.sort(v)[v.size // 2 if upper else (v.size - 1) // 2]


def block_rule(x, t, dt, ge=False, no_unit_rule=False):
    """block[block > t] = 1; block[block <= t] = 0"""
    if np.isnan(t):
        return x.copy()
    on = (x >= t) if ge else (x > t)
    if not no_unit_rule:
        on = on & (t < 1)
    return on.astype(dt)


def grad_mask_model(img, edge_threshold, dataset_type, dt=np.float64, pad="reflect", centre_only=False, upper=False, ge=False,
                    no_unit_rule=False, threshold_remainder=False):
    """-> dict(grad_v, grad_h, valid, intensity [H,W], out [H,W] (dt for replica, bool otherwise), thresholds ([32,32] or scalar)).
    The keyword arguments select the wrong models."""
    g = gray_of(img, dt)
    gv, gh = gradients(g, dt, pad)
    valid = validity(g, dt, EPS, pad, centre_only)
    x = intensity_of(gv, gh, valid, dt)
    H, W = x.shape
    thr = dt(np.float32(edge_threshold))
    res = dict(grad_v=gv, grad_h=gh, valid=valid, intensity=x)
    with np.errstate(invalid="ignore"):
        if dataset_type == "replica":
            bh, bw = H // BLOCKS, W // BLOCKS
            out = x.copy()
            ts = np.empty((BLOCKS, BLOCKS), dt)
            for r in range(BLOCKS):
                for c in range(BLOCKS):
                    blk = x[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
                    t = lower_median(blk, upper) * thr
                    ts[r, c] = t
                    out[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw] = block_rule(blk, t, dt, ge, no_unit_rule)
            if threshold_remainder:
                t = lower_median(x, upper) * thr
                rem = np.ones((H, W), bool)
                rem[:BLOCKS * bh, :BLOCKS * bw] = False
                out[rem] = block_rule(x[rem], t, dt, ge, no_unit_rule)
            res.update(out=out, thresholds=ts)
        else:
            t = lower_median(x, upper) * thr
            res.update(out=(x >= t) if ge else (x > t), thresholds=t)
    return res


WRONG_MASK_MODELS = {
    "replicate padding": dict(pad="edge"),
    "validity from the centre pixel": dict(centre_only=True),
    "x >= t": dict(ge=True),
    "no t < 1 rule": dict(no_unit_rule=True),
    "remainder thresholded": dict(threshold_remainder=True),
}


def block_region(H, W):
    """bool [H,W]: the pixels inside the 32 x 32 blocks (the rest keeps the raw intensity)"""
    m = np.zeros((H, W), bool)
    m[:BLOCKS * (H // BLOCKS), :BLOCKS * (W // BLOCKS)] = True
    return m


def block_thresholds_map(ts, H, W):
    """[32,32] thresholds spread over the block region of an H x W frame (NaN outside)"""
    bh, bw = H // BLOCKS, W // BLOCKS
    full = np.full((H, W), np.nan, np.float64)
    full[:BLOCKS * bh, :BLOCKS * bw] = np.kron(np.asarray(ts, np.float64), np.ones((bh, bw)))
    return full


def decided_region(name, oracle):
    """bool [H,W]: where the output of the case is a 0 / 1 decision (inside a block whose threshold is not NaN; everywhere for the frame
    median unless it is NaN), and the oracle's threshold at every pixel"""
    c = CASES[name]
    H, W = c["H"], c["W"]
    if c["type"] == "replica":
        tmap = block_thresholds_map(oracle["thresholds"], H, W)
        return block_region(H, W) & ~np.isnan(tmap), tmap
    t = float(oracle["thresholds"])
    return np.full((H, W), not np.isnan(t)), np.full((H, W), t)


def near_threshold(name, oracle, bound):
    """Pixels of the decided region whose 0 / 1 decision rounding may move: the float64 oracle puts x within ex + et of t, where ex is the
    bound on x and et = edge_threshold * bound that on t.  An intensity that is +0 because the pixel is invalid is exact in every
    implementation (0 * finite, squared, summed, rooted), so ex = 0 at an invalid pixel and et = 0 where the median itself is such a zero;
    a comparison of two exact numbers (ex + et = 0) cannot move.  Nor can that of a block of one pixel: the pixel is its own median, so every
    implementation compares its x with edge_threshold * x.  In the Replica branch the output is (x > t && t < 1): beyond et above 1 it is
    0 whatever x is, and within et of 1 it can move wherever x may exceed t."""
    c = CASES[name]
    decided, tmap = decided_region(name, oracle)
    x = oracle["intensity"]
    with np.errstate(invalid="ignore"):
        ex = np.where(oracle["valid"], bound, 0.0)
        et = np.where(tmap != 0, c["thr"] * bound, 0.0)
        near = (np.abs(x - tmap) <= ex + et) & (ex + et > 0)
        if c["type"] == "replica":
            near = (near & (tmap < 1 + et)) | ((np.abs(tmap - 1) <= et) & (x > tmap - (ex + et)))
    if c["type"] == "replica" and (c["H"] // BLOCKS) * (c["W"] // BLOCKS) == 1:
        near[:] = False
    return decided & near


# ---- the fixture's side of the bounds (golden: dict of tests/golden/image_ops.npz) ----
def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


def reference_intensity(golden, name, oracle):
    """the reference's own float32 intensity: sqrt((gv * mask)^2 + (gh * mask)^2) of its gradients and mask, and where its output keeps
    the raw intensity (the remainder, blocks with a NaN), that output itself"""
    c = CASES[name]
    gv, gh = golden[f"mask__{name}__grad_v"], golden[f"mask__{name}__grad_h"]
    valid = unpack(golden[f"mask__{name}__valid"], (c["H"], c["W"]))
    x = intensity_of(gv, gh, valid, np.float32)
    if c["type"] == "replica":
        decided, _ = decided_region(name, oracle)
        x[~decided] = golden[f"mask__{name}__out"][~decided]
    return x


def intensity_bound(golden, name, oracle):
    c = CASES[name]
    if c["golden"] == "packed":
        err = golden[f"mask__{name}__err"]
        return max(MARGIN * float(err[2]), ulp32(err[3]))
    return map_bound(reference_intensity(golden, name, oracle), oracle["intensity"])


# =================================================================================================================================
# masked medians
# =================================================================================================================================
def _depth_300x400(seed):
    rng = np.random.default_rng(seed)
    depth = (2.0 + rng.standard_normal((1, 300, 400)) * 0.7).astype(np.float32)
    depth[0, :40] = 0.0                                  # holes
    depth[0, 100:120, 50:90] = -1.0
    opacity = rng.uniform(0.85, 1.0, depth.shape).astype(np.float32)
    mask = rng.uniform(size=depth.shape) < 0.7
    return depth, opacity, mask


def median_case(name):
    """-> dict(depth [1,H,W] float32, opacity or None, mask or None).  get_median_depth selects depth > 0 (& opacity > 0.95 & mask)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    one = np.float32(1.5)
    bits = one.view(np.uint32)
    if name == "all_equal":
        d = np.full((1, 7, 9), one, np.float32)
    elif name == "lowest_byte":          # keys that differ in the last digit pass only
        d = (bits + rng.integers(0, 256, (1, 20, 25)).astype(np.uint32)).view(np.float32)
    elif name == "highest_byte":         # ... in the first only: 2^e for exponents that change bits 24..30
        d = np.ldexp(np.float32(1.0), rng.integers(-40, 40, (1, 20, 25)) * 2).astype(np.float32)
    elif name == "even_count":
        d = rng.uniform(0.5, 4.0, (1, 10, 10)).astype(np.float32)
    elif name == "odd_count":
        d = rng.uniform(0.5, 4.0, (1, 9, 11)).astype(np.float32)
    elif name == "count_1":
        d = np.zeros((1, 6, 5), np.float32)
        d[0, 2, 3] = 2.25
    elif name == "count_0":
        d = -np.abs(rng.standard_normal((1, 6, 5))).astype(np.float32)
    elif name == "depth_300x400":
        d, o, m = _depth_300x400(5)
        return dict(depth=d, opacity=o, mask=m)
    else:
        raise KeyError(name)
    return dict(depth=d, opacity=None, mask=None)


MEDIAN_CASES = ("all_equal", "lowest_byte", "highest_byte", "even_count", "odd_count", "count_1", "count_0", "depth_300x400")
MEDIAN_GOLDEN = tuple(n for n in MEDIAN_CASES if n != "count_0")     # the reference raises on an empty selection


def negative_values(seed=3, rows=2, n=1001):
    """values of both signs for masked_median (get_median_depth drops everything <= 0)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)


def median_model(depth, opacity=None, mask=None, upper=False, biased=False, positive_only=True):
    """-> (median float32, std float64, valid bool): the selection, its lower median bit for bit, its unbiased std in float64"""
    depth = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        valid = depth > 0 if positive_only else np.ones(depth.shape, bool)
        if opacity is not None:
            valid = valid & (np.asarray(opacity, np.float32) > np.float32(0.95))
    if mask is not None:
        valid = valid & np.asarray(mask, bool)
    sel = depth[valid]
    if sel.size == 0:
        return np.float32(np.nan), float("nan"), valid
    med = lower_median(sel, upper)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.std(sel.astype(np.float64), ddof=0 if biased else 1)) if sel.size > 1 or biased else float("nan")
    return med, std, valid


def std_bound(ref32, oracle64):
    """MARGIN * the reference's own float32 error, floored at one float32 ulp of the value (the device's std is a float32)"""
    if np.isnan(oracle64):
        return 0.0
    return max(MARGIN * abs(float(ref32) - float(oracle64)), ulp32(oracle64))
