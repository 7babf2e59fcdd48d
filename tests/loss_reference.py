"""Cases, bounds and wrong models for the loss stage (csrc/losses.hip) at its tile, mask and saturation edges: the fused mapping loss,
the L1 + SSIM colour-refinement loss and the PSNR / SSIM metrics of eval_rendering.  No GPU import.

  tests/golden/make_golden_loss_edges.py   runs the reference's own float32 functions on every case below and records values and autograd
                                           gradients (tests/golden/loss_edges.npz); the inputs are NOT stored: the builders here are seeded
                                           and the fixture holds a checksum of every case's inputs
  tests/test_host_loss_edges.py            fixture against the float64 oracle (oracle/losses.py), every case reaches the edge it names, every
                                           wrong model below deviates by more than the bound on the case named for it
  tests/test_gpu_loss_edges.py             the kernels against the float64 oracle within the bounds below

Bounds are functions of the case (`bound()`): E_ref(case) = max-norm deviation of the reference's float32 result (the fixture) from the
float64 oracle; the device may deviate by MARGIN * E_ref.  MARGIN is 4 because the kernels' separable float32 blur sums in another
order than the reference's dense 121-tap convolution: it need not land closer than the reference, but has no reason to be several
times worse.  Scalars are floored at one float32 ulp of the value (the kernels round a double sum to float once); the combined loss at
the ulps of the two means it is formed from (`loss_floor`); a map at one ulp of its largest element, dL/dmarker at two ulps of the
sigmoid over HW (`map_bound`, `marker_bound`: on a map of one pixel E_ref is 0 as often as not).  Each floor is argued where it is defined.

The builders use only IEEE float32 arithmetic on np.random.RandomState uniforms (no libm call), so that they reproduce bit for bit.
"""
import hashlib
import zlib

import numpy as np

from oracle import losses as OL

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: one ulp of 1.0f
MARGIN = 4.0
RH = 5                                            # window radius
FW, FH = 32, 16                                   # tile of refine_fwd / refine_bwd
ET = 16                                           # tile edge of eval_metrics_kernel
BLOCK = 256                                       # LOSS_BLOCK: block of the mapping loss and of every finish loop
MAX_LOSS_BLOCKS = 2048
LAMBDAS = (0.2, 1.0, 0.0)
W64 = OL.gaussian_window().astype(np.float64)


def _seed(name):
    return zlib.crc32(name.encode())


def _noise(rs, shape):
    """unit-variance bell-shaped noise without libm: an Irwin-Hall sum of four uniforms"""
    return ((rs.rand(4, *shape).sum(axis=0) - 2.0) * np.sqrt(3.0)).astype(F32)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest()[:16], dtype=np.uint8).copy()


def ulp32(v):
    """one float32 ulp at the value v"""
    return float(np.spacing(np.abs(F32(v))))


def ulps_apart(a, b):
    """elementwise distance of two float32 arrays in units in the last place (of their ordered integer images); +0 and -0 are 0 apart"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def exceeds(dev, bound):
    """a deviation that is NOT within the bound (NaN and inf exceed every bound)"""
    return not (dev <= bound)


# =================================================================================================================================
# refinement loss
# =================================================================================================================================
REFINE_SHAPES = ((1, 1, 1), (1, 5, 5), (3, 6, 6), (3, 16, 32), (3, 17, 33), (3, 15, 31), (1, 16, 37), (3, 21, 43),
                 (3, 1400, 1), (3, 1, 2752), (4, 17, 33))
CONTENT_SHAPE = (3, 37, 53)
CONTENTS = ("noise", "smooth_converged", "flat_offset", "flat_equal", "black", "l1_ties")


def shape_name(shape):
    return "shape %dx%dx%d" % tuple(shape)


def refine_case_names():
    return [shape_name(s) for s in REFINE_SHAPES] + ["content " + c for c in CONTENTS]


def refine_blocks(C, H, W):
    return -(-W // FW) * -(-H // FH) * C


def eval_blocks(C, H, W):
    return -(-W // ET) * -(-H // ET) * C


def _noise_pair(rs, shape):
    gt = rs.rand(*shape).astype(F32)
    image = np.clip(gt + F32(0.15) * _noise(rs, shape), F32(0), F32(1)).astype(F32)
    return image, gt


def l1_tie_positions(H, W):
    """(y, x) of the exact zeros of x - y in `l1_ties`: the four corners and both sides of every 32x16 tile seam"""
    pos = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    for ys in range(FH, H, FH):
        pos |= {(y, x) for y in (ys - 1, ys) for x in range(0, W, 3)}
    for xs in range(FW, W, FW):
        pos |= {(y, x) for x in (xs - 1, xs) for y in range(0, H, 2)}
    return sorted(pos)


def refine_case(name):
    """dict(name, image, gt [C,H,W] float32, edge): `edge` names what the case is there for"""
    rs = np.random.RandomState(_seed(name))
    if name.startswith("shape "):
        shape = tuple(int(v) for v in name.split()[1].split("x"))
        image, gt = _noise_pair(rs, shape)
        C, H, W = shape
        edge = dict(tiles=(-(-H // FH), -(-W // FW)), blocks=refine_blocks(*shape), last_rows=(H - 1) % FH + 1, last_cols=(W - 1) % FW + 1)
    else:
        kind = name.split(" ", 1)[1]
        shape = CONTENT_SHAPE
        C, H, W = shape
        edge = dict(kind=kind)
        if kind in ("noise", "l1_ties"):
            image, gt = _noise_pair(rs, shape)
            if kind == "l1_ties":
                for (y, x) in l1_tie_positions(H, W):
                    image[:, y, x] = gt[:, y, x]
        elif kind == "smooth_converged":
            v, u = np.meshgrid(np.arange(H, dtype=F32) / F32(H - 1), np.arange(W, dtype=F32) / F32(W - 1), indexing="ij")
            base = F32(0.72) + F32(0.15) * (F32(4) * u * (F32(1) - u)) * (F32(1) - v * v * F32(0.5))
            gt = np.stack([base + F32(0.03) * F32(c) for c in range(C)]).astype(F32)
            image = (gt + F32(1e-3) * _noise(rs, shape)).astype(F32)
        elif kind == "flat_offset":
            gt = np.full(shape, 0.9, F32)
            image = (gt + F32(1e-3) * _noise(rs, shape)).astype(F32)
        elif kind == "flat_equal":
            gt = np.full(shape, 0.9, F32)
            image = gt.copy()
        elif kind == "black":
            gt = np.zeros(shape, F32)
            image = gt.copy()
        else:
            raise KeyError(name)
    assert image.dtype == F32 and gt.dtype == F32 and image.shape == shape
    return dict(name=name, image=image, gt=gt, edge=edge)


# ---- the float64 model of the loss with a choice of defects (none: the oracle restated) ---------------------------------------------
def fetch_zero(a, gy, gx):
    H, W = a.shape[-2:]
    ok = (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W)
    return a[..., np.clip(gy, 0, H - 1), np.clip(gx, 0, W - 1)] * ok


def fetch_replicate(a, gy, gx):
    H, W = a.shape[-2:]
    return a[..., np.clip(gy, 0, H - 1), np.clip(gx, 0, W - 1)]


def fetch_row_wrap(a, gy, gx):
    """a loader without its `gx < W` guard: right of the image it reads on in memory, the next row's first pixels (the next plane's after
    the last row; nothing is modelled behind the last plane: zero)"""
    C, H, W = a.shape
    flat = np.concatenate([a.reshape(-1), np.zeros(W + 2 * RH + FW)])
    ok = (gy >= 0) & (gy < H) & (gx >= 0)
    idx = (np.arange(C)[:, None, None] * H + np.clip(gy, 0, H - 1)[None]) * W + np.clip(gx, 0, None)[None]
    return flat[np.minimum(idx, len(flat) - 1)] * ok


def fetch_short_halo(th, tw, halo=RH - 1):
    """a tile loader whose halo is one ring short: an output sees only the sources within `halo` of its own th x tw tile"""
    def fetch(a, gy, gx, oy, ox):
        ty0, tx0 = (oy // th) * th, (ox // tw) * tw
        ok = (gy >= ty0 - halo) & (gy < ty0 + th + halo) & (gx >= tx0 - halo) & (gx < tx0 + tw + halo)
        return fetch_zero(a, gy, gx) * ok
    fetch.wants_output = True
    return fetch


def blur(a, fetch=fetch_zero):
    """the 11x11 window as 121 dense taps over a [C,H,W] float64 array, its sources read through `fetch`"""
    a = np.asarray(a, np.float64)
    H, W = a.shape[-2:]
    oy, ox = np.mgrid[0:H, 0:W]
    out = np.zeros_like(a)
    for dy in range(-RH, RH + 1):
        for dx in range(-RH, RH + 1):
            src = fetch(a, oy + dy, ox + dx, oy, ox) if getattr(fetch, "wants_output", False) else fetch(a, oy + dy, ox + dx)
            out += W64[dy + RH] * W64[dx + RH] * src
    return out


def tile_mean_of_means(m, th=FH, tw=FW):
    C, H, W = m.shape
    return float(np.mean([m[c, y:y + th, x:x + tw].mean() for c in range(C) for y in range(0, H, th) for x in range(0, W, tw)]))


def refine_model(image, gt, lam, fwd=fetch_zero, bwd=fetch_zero, tile_mean=False):
    """oracle.losses.refinement_loss restated over `blur`; dict(l1, ssim, loss, dL_dimage, partial_blurs)"""
    x, y = np.asarray(image, np.float64), np.asarray(gt, np.float64)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = blur(x, fwd), blur(y, fwd)
    s1, s2, s12 = blur(x * x, fwd), blur(y * y, fwd), blur(x * y, fwd)
    sig1, sig2, sig12 = s1 - mu1 * mu1, s2 - mu2 * mu2, s12 - mu1 * mu2
    A, B = 2 * mu1 * mu2 + C1, 2 * sig12 + C2
    Cc, D = mu1 * mu1 + mu2 * mu2 + C1, sig1 + sig2 + C2
    m = A * B / (Cc * D)
    n = x.size
    l1 = float(np.abs(x - y).mean())
    ssim = tile_mean_of_means(m) if tile_mean else float(m.mean())
    dm_dmu1 = (2 * mu2 * (B - A) * Cc * D - A * B * 2 * mu1 * (D - Cc)) / (Cc * D) ** 2
    dm_ds1 = -A * B / (Cc * D * D)
    dm_ds12 = 2 * A / (Cc * D)
    pb = (blur(dm_dmu1, bwd), blur(dm_ds1, bwd), blur(dm_ds12, bwd))
    grad = (1.0 - lam) * np.sign(x - y) / n - lam * (pb[0] + 2 * x * pb[1] + y * pb[2]) / n
    return dict(l1=l1, ssim=ssim, loss=(1.0 - lam) * l1 + lam * (1.0 - ssim), dL_dimage=grad, partial_blurs=pb)


REFINE_WRONG = {
    # model: (keyword arguments of refine_model, the case named for it, the lambda, what it moves)
    "forward halo one ring short": (dict(fwd=fetch_short_halo(FH, FW)), "content noise", 1.0, "dL_dimage"),
    "backward halo one ring short": (dict(bwd=fetch_short_halo(FH, FW)), "content noise", 1.0, "dL_dimage"),
    "forward halo short, converged": (dict(fwd=fetch_short_halo(FH, FW)), "content smooth_converged", 0.2, "dL_dimage"),
    "replicate padding": (dict(fwd=fetch_replicate, bwd=fetch_replicate), "shape 1x5x5", 0.2, "dL_dimage"),
    "no gx < W guard": (dict(fwd=fetch_row_wrap), "shape 3x17x33", 0.2, "dL_dimage"),
    "no gx < W guard, backward": (dict(bwd=fetch_row_wrap), "shape 3x15x31", 0.2, "dL_dimage"),
    "mean of tile means": (dict(tile_mean=True), "shape 3x17x33", 0.2, "ssim"),
}


def flat_equal_grad_bound(image, gt, lam):
    """`flat_equal`: image == gt, the gradient is 0 in exact arithmetic and E_ref is arbitrarily small, so the bound is absolute: the
    three blurred partials cancel, each known to a relative float32 rounding, MARGIN roundings in all"""
    o = refine_model(image, gt, lam)
    pb = o["partial_blurs"]
    x, y = np.asarray(image, np.float64), np.asarray(gt, np.float64)
    return MARGIN * EPS32 * lam / x.size * float((np.abs(pb[0]) + 2 * np.abs(x) * np.abs(pb[1]) + np.abs(y) * np.abs(pb[2])).max())


def scalar_bound(ref32, oracle64):
    """MARGIN * |ref32 - oracle64|, floored at one float32 ulp of the value"""
    return max(MARGIN * abs(float(ref32) - float(oracle64)), ulp32(oracle64))


def loss_floor(lam, l1, ssim):
    """The floor of the combined loss (1 - lambda) l1 + lambda (1 - ssim): it is formed from the two means, each good to one float32 ulp of
    itself at best, so it cannot be asked for more than that; one ulp of the loss's own value would ask flat_equal (loss 0, ssim 1) for a
    1 - ssim within 1e-45 while its ssim is allowed one ulp of 1."""
    return (1.0 - lam) * ulp32(l1) + lam * ulp32(ssim)


def map_bound(ref32, oracle64):
    """MARGIN * E_ref for a per-pixel map, floored at one float32 ulp of the map's largest element: the device's map is a float32 too, and
    on a map of one pixel the reference's E_ref can be 0 by chance"""
    oracle64 = np.asarray(oracle64, np.float64)
    return max(MARGIN * float(np.abs(np.asarray(ref32, np.float64).reshape(oracle64.shape) - oracle64).max()), ulp32(np.abs(oracle64).max()))


def marker_bound(ref32, oracle64):
    """the same for dL/dmarker = (s - y) / HW, floored at one ulp of s = sigmoid(z) in [0.5, 1) doubled, over HW: expf on the device is
    within 1 ulp and the division rounds once more, whatever y is (on one pixel E_ref is 0 as often as not)"""
    oracle64 = np.asarray(oracle64, np.float64)
    return max(map_bound(ref32, oracle64), EPS32 / oracle64.size)


# =================================================================================================================================
# eval metrics
# =================================================================================================================================
EVAL_SHAPES = ((3, 33, 47), (1, 1, 1), (3, 16, 16), (3, 17, 17), (1, 5, 40))
TINY = np.finfo(np.float32).tiny                   # the smallest normal float32
SUBNORMAL = F32(1e-40)
# (render, gt) pairs laid over the noise: renders below 0, exactly 0, exactly 1, above 1, far above 1; gt exactly 0, the smallest normal,
# a subnormal (the reference's mask counts it: 1e-40 > 0)
EVAL_SPECIALS = ((1.5, 0.5), (-0.25, 0.5), (0.0, 0.5), (1.0, 0.5), (1e6, 0.5), (0.5, 0.0), (0.5, TINY), (0.5, SUBNORMAL), (1.5, 0.0),
                 (-0.25, SUBNORMAL), (1.0, 1.0), (0.0, TINY))


def eval_case_names():
    return [shape_name(s) for s in EVAL_SHAPES] + ["single element mask", "identical", "empty mask", "channel zero"]


def eval_case(name):
    """dict(name, render, gt [C,H,W] float32, edge)"""
    rs = np.random.RandomState(_seed("eval " + name))
    if name.startswith("shape "):
        shape = tuple(int(v) for v in name.split()[1].split("x"))
        gt = (F32(0.05) + F32(0.9) * rs.rand(*shape)).astype(F32)
        render = (gt + F32(0.2) * _noise(rs, shape)).astype(F32)           # un-clamped: leaves [0, 1] on its own, too
        n = gt.size
        stride = max(1, n // len(EVAL_SPECIALS))
        placed = []
        for k, (r, g) in enumerate(EVAL_SPECIALS):
            p = k * stride + (k % 3 if stride > 3 else 0)
            if p < n:
                render.reshape(-1)[p], gt.reshape(-1)[p] = F32(r), F32(g)
                placed.append(p)
        edge = dict(placed=placed, blocks=eval_blocks(*shape))
    else:
        shape = (3, 17, 17)
        gt = (F32(0.05) + F32(0.9) * rs.rand(*shape)).astype(F32)
        render = (gt + F32(0.2) * _noise(rs, shape)).astype(F32)
        edge = dict(blocks=eval_blocks(*shape))
        if name == "single element mask":
            gt[:] = 0
            gt[1, 16, 16] = F32(0.625)                                       # the last tile's one pixel
        elif name == "identical":
            render = gt.copy()
        elif name == "empty mask":
            gt[:] = 0
        elif name == "channel zero":
            gt[1, :, 5:12] = 0                                              # one channel only: the mask is per element, not per pixel
        else:
            raise KeyError(name)
    return dict(name=name, render=render, gt=gt, edge=edge)


def eval_model(render, gt, fetch=fetch_zero, clamp=True, mask="gt > 0"):
    """oracle.losses.eval_metrics restated over `blur` with a choice of defects; dict(psnr, ssim, mse, count)"""
    x = np.asarray(render, np.float64)
    if clamp:
        x = np.clip(x, 0.0, 1.0)
    y = np.asarray(gt, np.float64)
    msk = {"gt > 0": y > 0, "gt >= 0": y >= 0, "per pixel": np.broadcast_to((y > 0).any(axis=0, keepdims=True), y.shape)}[mask]
    count = int(msk.sum())
    mse = float(((x[msk] - y[msk]) ** 2).mean()) if count else float("nan")
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = blur(x, fetch), blur(y, fetch)
    sig1, sig2, sig12 = blur(x * x, fetch) - mu1 * mu1, blur(y * y, fetch) - mu2 * mu2, blur(x * y, fetch) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * sig12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (sig1 + sig2 + C2))
    with np.errstate(divide="ignore"):
        psnr = float(20.0 * np.log10(1.0 / np.sqrt(mse))) if count else float("nan")
    return dict(psnr=psnr, ssim=float(m.mean()), mse=mse, count=count)


EVAL_WRONG = {
    # model: (keyword arguments of eval_model, the case named for it, the outputs it must move)
    "eval halo one ring short": (dict(fetch=fetch_short_halo(ET, ET)), "shape 3x33x47", ("ssim",)),
    "eval without the clamp": (dict(clamp=False), "shape 3x16x16", ("ssim", "mse")),
    "eval mask >=": (dict(mask="gt >= 0"), "shape 3x17x17", ("count", "mse")),
    "eval mask per pixel": (dict(mask="per pixel"), "channel zero", ("count", "mse")),
}


# =================================================================================================================================
# mapping loss
# =================================================================================================================================
THR = F32(0.01)                                   # rgb_boundary_threshold; the depth threshold of utils/utils.py:75 is the same number
MAPPING_HW = (1, 63, 64, 255, 256, 257, 4801)
GRID_STRIDE_HW = MAX_LOSS_BLOCKS * BLOCK + 257    # oracle only: 257 threads of the 2048 blocks take a second pixel (a block and one)
TIE_HW = 257
EXPOSURES = {"none": None, "ab": (0.13, -0.04), "zero": (0.0, 0.0)}
LOGITS = (0.0, 16.6, -16.6, 17.0, -17.0, 88.0, -88.0, 89.0, -89.0, 1e4, -1e4)
SOFT_TARGETS = (0.0, 1.0, 1e-6, 0.999)
RGB_TIE_KINDS = ("exact", "below", "above", "left side only", "right side only", "ordinary")
DEPTH_TIE_KINDS = ("exact", "below", "above", "ordinary")


def mapping_case_names():
    return ["hw %d" % n for n in MAPPING_HW] + ["rgb ties", "depth ties", "l1 zeros", "marker saturation"]


def _sum3(t0, t1, t2):
    return F32(F32(t0 + t1) + t2)


def rgb_tie_triples(rs):
    """float32 triples by kind: (t0+t1)+t2 exactly THR, one ulp below, one ulp above, and two for which (t0+t1)+t2 and t0+(t1+t2) fall on
    different sides of THR (the reference and the kernel both sum left to right)"""
    up, down = np.nextafter(THR, F32(1)), np.nextafter(THR, F32(0))
    out = {}
    while len(out) < 5:
        t0, t1 = (F32(0.004) * rs.rand(2).astype(F32)).astype(F32)
        t2 = F32(THR - F32(t0 + t1))
        for _ in range(8):                           # walk t2 by ulps: its ulp is no larger than the sum's
            left, right = _sum3(t0, t1, t2), F32(t0 + F32(t1 + t2))
            for kind, want in (("exact", THR), ("below", down), ("above", up)):
                if kind not in out and left == want:
                    out[kind] = (t0, t1, t2)
            if "left side only" not in out and left > THR and not right > THR:
                out["left side only"] = (t0, t1, t2)
            if "right side only" not in out and right > THR and not left > THR:
                out["right side only"] = (t0, t1, t2)
            t2 = np.nextafter(t2, F32(1) if rs.rand() < 0.5 else F32(0))
    return out


def mapping_case(name):
    """dict(name, H, W, image [3,H,W], depth [1,H,W], marker [H,W], gt_image, gt_depth [H,W], kp [H,W], edge); every array float32, H = 1"""
    rs = np.random.RandomState(_seed("mapping " + name))
    HW = GRID_STRIDE_HW if name == "grid stride" else int(name.split()[1]) if name.startswith("hw ") else TIE_HW
    p = np.arange(HW)
    image = rs.rand(3, HW).astype(F32)
    depth = (F32(0.5) + F32(3) * rs.rand(HW)).astype(F32)
    scale, top = (F32(1.5), F32(4)) if name == "grid stride" else (F32(3), F32(30))   # oracle only: small |logit|, see bce_rounding_bound
    marker = np.clip(scale * _noise(rs, (HW,)), -top, top)
    gt_image = (F32(0.02) + rs.rand(3, HW)).astype(F32)
    gt_depth = (F32(0.5) + F32(3) * rs.rand(HW)).astype(F32)
    kp = (rs.rand(HW).astype(F32) ** 2).astype(F32) ** 2
    # every size case: masked pixels, invalid depths and exact L1 zeros, spread so that the ragged tail holds some
    gt_image[:, p % 8 == 3] = 0
    gt_depth[p % 8 == 5] = 0
    zeros = p % 16 == 9
    image[:, zeros] = gt_image[:, zeros]
    depth[zeros] = gt_depth[zeros]
    edge = dict(HW=HW, blocks=min(-(-HW // BLOCK), MAX_LOSS_BLOCKS), tail=HW % BLOCK)
    if name == "rgb ties":
        triples = rgb_tie_triples(rs)
        kinds = np.array([k % len(RGB_TIE_KINDS) for k in p])
        for k, kind in enumerate(RGB_TIE_KINDS[:-1]):
            gt_image[:, kinds == k] = np.array(triples[kind], F32)[:, None]
        edge.update(kinds=kinds, triples=triples)
    elif name == "depth ties":
        kinds = np.array([k % len(DEPTH_TIE_KINDS) for k in p])
        for k, v in enumerate((THR, np.nextafter(THR, F32(0)), np.nextafter(THR, F32(1)))):
            gt_depth[kinds == k] = v
        edge.update(kinds=kinds)
    elif name == "l1 zeros":
        zeros = p % 3 == 0
        image[:, zeros] = gt_image[:, zeros]
        depth[zeros] = gt_depth[zeros]
        edge.update(zeros=zeros)
    elif name == "marker saturation":
        marker = np.array([LOGITS[k % len(LOGITS)] for k in p], F32)
        kp = np.array([SOFT_TARGETS[(k // len(LOGITS)) % len(SOFT_TARGETS)] for k in p], F32)
    return dict(name=name, H=1, W=HW, image=image.reshape(3, 1, HW), depth=depth.reshape(1, 1, HW), marker=marker.reshape(1, HW),
                gt_image=gt_image.reshape(3, 1, HW), gt_depth=gt_depth.reshape(1, HW), kp=kp.reshape(1, HW), edge=edge)


def mapping_inputs(c):
    return tuple(c[k] for k in ("image", "depth", "marker", "gt_image", "gt_depth", "kp"))


def mapping_model(c, exposure, mask_ge=False, drop_tail=False, no_clamp=False, masked_mean=False):
    """oracle.losses.mapping_loss restated with a choice of defects (none: the oracle, bit for bit)"""
    image, depth, marker, gt_image, gt_depth, y = (np.asarray(a, F32) for a in mapping_inputs(c))
    H, W = marker.shape
    gt_depth = gt_depth.reshape(depth.shape)
    use_exp = exposure is not None
    ea = F32(np.exp(np.float64(F32(exposure[0])))) if use_exp else F32(1.0)
    eb = F32(exposure[1]) if use_exp else F32(0.0)
    x = ea * image + eb if use_exp else image
    s3 = gt_image.sum(axis=0)
    m_rgb = ((s3 >= THR) if mask_ge else (s3 > THR)).reshape(1, H, W).astype(F32)
    m_d = ((gt_depth >= THR) if mask_ge else (gt_depth > THR)).astype(F32)
    live = np.ones((1, H, W))
    if drop_tail:
        live.reshape(-1)[(H * W // BLOCK) * BLOCK:] = 0
    diff, diffd = (x * m_rgb - gt_image * m_rgb) * live, (depth * m_d - gt_depth * m_d) * live
    n_rgb, n = 3.0 * H * W, 1.0 * H * W
    if masked_mean:
        n_rgb, n_d = 3.0 * max(m_rgb.sum(), 1.0), max(m_d.sum(), 1.0)
    else:
        n_d = n
    l_rgbd = np.abs(diff).sum(dtype=np.float64) / n_rgb + np.abs(diffd).sum(dtype=np.float64) / n_d
    with np.errstate(over="ignore"):
        e = np.exp(-marker.astype(np.float64)).astype(F32)
        p = (F32(1.0) / (F32(1.0) + e)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        logp, log1p = np.log(p.astype(np.float64)), np.log((F32(1.0) - p).astype(np.float64))
        if not no_clamp:
            logp, log1p = np.maximum(logp, -100.0), np.maximum(log1p, -100.0)
        l_bce = ((-(y * logp + (1.0 - y) * log1p)) * live[0]).sum(dtype=np.float64) / n
    g_x = np.sign(diff).astype(np.float64) * m_rgb / n_rgb
    p64 = p.astype(np.float64)
    g_marker = (p64 - y) / np.maximum((1.0 - p64) * p64, 1e-12) * (p64 * (1.0 - p64)) / n * live[0]
    return dict(loss_rgbd=l_rgbd, loss_bce=l_bce, dL_dimage=g_x * float(ea), dL_ddepth=np.sign(diffd).astype(np.float64) * m_d / n_d,
                dL_dmarker=g_marker, dL_dexposure_a=float((g_x * image).sum() * float(ea)) if use_exp else 0.0,
                dL_dexposure_b=float(g_x.sum()) if use_exp else 0.0)


MAPPING_WRONG = {
    # model: (keyword arguments of mapping_model, the case named for it, the outputs it must move)
    "rgb mask >= at the tie": (dict(mask_ge=True), "rgb ties", ("dL_dimage", "loss_rgbd")),
    "depth mask >= at the tie": (dict(mask_ge=True), "depth ties", ("dL_ddepth", "loss_rgbd")),
    "tail of HW % 256 pixels dropped": (dict(drop_tail=True), "hw 257", ("dL_dimage", "dL_ddepth", "dL_dmarker", "loss_rgbd", "loss_bce")),
    "tail dropped below one block": (dict(drop_tail=True), "hw 63", ("dL_dimage", "dL_ddepth", "dL_dmarker", "loss_rgbd", "loss_bce")),
    "BCE without the -100 clamp": (dict(no_clamp=True), "marker saturation", ("loss_bce",)),
    "L1 mean over the masked count": (dict(masked_mean=True), "hw 4801", ("dL_dimage", "dL_ddepth", "loss_rgbd")),
}

# Elementwise bounds of the mapping gradients, in ulps of the reference's float32 element.
#   g_depth = sign(dd) * md * (1 / HW): the reference's autograd divides 1 by HW (exact below 2^24, one correctly rounded division) and
#       multiplies by the sign and the mask (exact).  The kernel does the same: 0 roundings may differ; the bound is 1 ulp.
#   g_image = sign(diff) * m * (1 / (3 HW)) * exp(a): the same exact factor, times exp(a).  expf on the device and torch.exp on the CPU are
#       each within 1 ulp of exp(a) and may differ from one another by 1 ulp (1 rounding); the product with 1 / (3 HW) rounds once more, and
#       that rounding can fall either way once its argument moved (1 rounding): 2 roundings may differ, the bound is 2 ulp.  Without the
#       exposure pair, and at a = 0, exp(a) is exactly 1 and the elements are equal.
G_DEPTH_ULPS = 1
G_IMAGE_ULPS = 2


def bce_rounding_bound(marker, kp):
    """An a-priori bound on |device BCE mean - oracle BCE mean| where no fixture exists (the grid-stride case).  s = 1 / (1 + exp(-z)) is
    three float32 roundings from exact (expf, the sum, the division: 3u, u = 2^-23 covering a 1-ulp expf); log(s) moves by 3u, log(1 - s) by
    3u s / (1 - s), and each logarithm adds 1 ulp of its value.  The oracle's own float32 s is as far off: twice that."""
    z = np.asarray(marker, np.float64)
    y = np.asarray(kp, np.float64)
    s = 1.0 / (1.0 + np.exp(-z))
    u = EPS32
    per = y * (3 * u + u * np.abs(np.log(s))) + (1 - y) * (3 * u * s / (1 - s) + u * np.abs(np.log1p(-s)))
    return 2.0 * float(per.mean())


def l1_rounding_bound(c, exposure):
    """The same for the L1 term: every |x m - gt m| is at most three float32 roundings (exp(a), the affine, the difference) of magnitude
    u (|x| + |gt|); the depth term one; the sums are double."""
    ea = np.exp(exposure[0]) if exposure is not None else 1.0
    eb = exposure[1] if exposure is not None else 0.0
    x = np.abs(ea * c["image"].astype(np.float64)) + abs(eb)
    return EPS32 * float((3 * (x + np.abs(c["gt_image"])).mean() + (np.abs(c["depth"]) + np.abs(c["gt_depth"])).mean()))
