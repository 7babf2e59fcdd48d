"""What the dead marks of the forward (bits 28..31 of the payload word) may and must say, from the CPU oracle's
forward alone — no GPU, no product code.

For every (list entry, quadrant of its tile), from `xy`, `conic_opacity`, `point_list`, `ranges` and `n_contrib`:

  * `reach`        the conservative reach bit (composite_common.h quadrant_reach_mask restated in float32 numpy);
  * `walked`       reach bit set and the entry lies in front of the quadrant's last contributor: what the backward walks;
  * `must_not`     some pixel of the quadrant has `idx < n_contrib && pass`: a contributor — a mark here loses gradient;
  * `contributes`  the same with the alpha test decided the OTHER way at the threshold (see below): its complement inside
                   `walked` are the candidates without a contributing pixel;
  * `must_mark`    walked, and no pixel of the quadrant inside the image passes the alpha test at all, whatever its state: the
                   forward evaluated the entry (the quadrant was still accumulating: a contributor lies behind it) and no lane
                   could be live.

The alpha test alpha = o 2^power >= 1/255 is evaluated in float64 with libm's exp, not with the kernels' bit-exact 2^x; the two
differ by a few float32 roundings of the power (relative 1e-6 at |power| <= 6) and 1.4 ulp of 2^x, so a pixel within REL = 1e-5 of
the threshold is left undecided: `must_not` counts only pixels that pass by that margin, `must_mark` / `contributes` treat every
pixel that passes up to that margin as passing.  Both sets shrink, neither claims what the kernel's own rounding could undo.
"""
import numpy as np
import torch

from splatloc_amd.synthetic import make_scene

TILE = 16
REL = 1e-5
ALPHA_MIN = 1.0 / 255.0


def reach_mask(xy, con, tx0, ty0):
    """[n, 4] bool: quadrant_reach_mask in float32 (log and reciprocal: numpy's, within the test's own 0.02 + 1e-4 slack)"""
    f = np.float32
    A, B, Cc, o = (con[:, k].astype(f) for k in range(4))
    x, y = xy[:, 0].astype(f), xy[:, 1].astype(f)
    out = np.zeros((len(A), 4), bool)
    with np.errstate(all="ignore"):
        lim0 = f(2.0) * np.log(f(255.0) * o).astype(f)
        lim = lim0 + f(0.02) + f(1e-4) * np.abs(lim0)
        nBrA, nBrC = -B * (f(1.0) / A), -B * (f(1.0) / Cc)
        for q in range(4):
            bx0, by0 = f(tx0 + (q & 1) * 8), f(ty0 + (q >> 1) * 8)
            u0, u1 = x - (bx0 + f(7.0)), x - bx0
            v0, v1 = y - (by0 + f(7.0)), y - by0
            inside = (u0 <= 0) & (u1 >= 0) & (v0 <= 0) & (v1 >= 0)
            qmin = np.full(len(A), 3.0e38, f)
            for ue, ve in ((u0, v0), (u1, v1)):
                vs = np.minimum(v1, np.maximum(v0, nBrC * ue))
                qmin = np.minimum(qmin, A * ue * ue + f(2.0) * B * ue * vs + Cc * vs * vs)
                us = np.minimum(u1, np.maximum(u0, nBrA * ve))
                qmin = np.minimum(qmin, A * us * us + f(2.0) * B * us * ve + Cc * ve * ve)
            qmin = np.where(inside, f(0.0), qmin)
            out[:, q] = (qmin <= lim) & (lim > 0)
    return out


def dead_mark_sets(f, W, H, reach=None):
    """The sets above as [R, 4] bool arrays in list order (R = num_rendered), plus `pos` [R] (the entry's position in its list) and
    `tile` [R].  `reach`: [R, 4] reach bits to use instead of the restated ones (the stream's own, where a test has them)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    R = int(f["num_rendered"])
    keys = ("reach", "walked", "must_not", "contributes", "must_mark")
    out = {k: np.zeros((R, 4), bool) for k in keys}
    out["pos"] = np.zeros(R, np.int64)
    out["tile"] = np.zeros(R, np.int64)
    for t in range(gx * gy):
        s, e = (int(v) for v in f["ranges"][t])
        if e <= s:
            continue
        ty, tx = divmod(t, gx)
        g = f["point_list"][s:e].astype(np.int64)
        xy, con = f["xy"][g].astype(np.float64), f["conic_opacity"][g].astype(np.float64)
        out["pos"][s:e] = np.arange(e - s)
        out["tile"][s:e] = t
        rm = reach_mask(f["xy"][g], f["conic_opacity"][g], tx * TILE, ty * TILE) if reach is None else reach[s:e]
        ys, xs = np.mgrid[ty * TILE:ty * TILE + TILE, tx * TILE:tx * TILE + TILE]
        inside = (ys < H) & (xs < W)                                                      # [16, 16]
        nc = np.where(inside, f["n_contrib"][np.minimum(ys, H - 1), np.minimum(xs, W - 1)], 0).astype(np.int64)
        dx = xy[:, 0, None, None] - xs[None]
        dy = xy[:, 1, None, None] - ys[None]
        power = -0.5 * (con[:, 0, None, None] * dx * dx + con[:, 2, None, None] * dy * dy) - con[:, 1, None, None] * dx * dy
        with np.errstate(all="ignore"):
            alpha = con[:, 3, None, None] * np.exp(power)
        sure = (power <= -1e-6) & (alpha >= ALPHA_MIN * (1.0 + REL)) & inside[None]       # passes, whatever the rounding
        maybe = (power <= 1e-6) & (alpha >= ALPHA_MIN * (1.0 - REL)) & inside[None]       # may pass
        before = np.arange(e - s)[:, None, None] < nc[None]                               # idx < n_contrib
        for q in range(4):
            qs = (slice(None), slice((q >> 1) * 8, (q >> 1) * 8 + 8), slice((q & 1) * 8, (q & 1) * 8 + 8))
            last = int(nc[qs[1:]].max())
            walked = rm[:, q] & (np.arange(e - s) < last)
            out["reach"][s:e, q] = rm[:, q]
            out["walked"][s:e, q] = walked
            out["must_not"][s:e, q] = (sure & before)[qs].any(axis=(1, 2))
            out["contributes"][s:e, q] = (maybe & before)[qs].any(axis=(1, 2))
            out["must_mark"][s:e, q] = walked & ~maybe[qs].any(axis=(1, 2))
    return out


def quadrant_finish_chunks(f, W, H, t):
    """for tile t: per quadrant, the 64-entry chunk of the list that holds its last contributor (-1: none)"""
    gx = (W + TILE - 1) // TILE
    ty, tx = divmod(t, gx)
    out = []
    for q in range(4):
        y0, x0 = ty * TILE + (q >> 1) * 8, tx * TILE + (q & 1) * 8
        nc = f["n_contrib"][y0:min(y0 + 8, H), x0:min(x0 + 8, W)]
        last = int(nc.max()) if nc.size else 0
        out.append((last - 1) // 64 if last else -1)
    return out


# ---- the occluder scene -----------------------------------------------------------------------------------------------------------
# Everything sits in ONE tile (origin ox, oy) of a small frame; depth ranks are spread so that the tile's list of ~190 entries has
#   * 6 pixel-missing Gaussians in front of everything (dead entries at the head of chunk 0),
#   * a near layer: per quadrant in `finished`, 6 sheets of 2 x 2 Gaussians of sigma 3 px and opacity 0.99 (centres 4 px apart: every
#     pixel of the quadrant lies within 2.2 px of one, alpha >= 0.75 per sheet) — its pixels are finished (T < 1e-4) by the sheets,
#     within the list's first two chunks; the neighbouring quadrants are dimmed near the border, not finished,
#   * behind it 110 entries in random depth order: 60 % small Gaussians (sigma ~0.6 px after the 0.3 px^2 dilation) of opacity 0.5
#     anywhere in the tile — footprints wholly or partly on finished pixels, and the deep contributors of the open quadrants —, 40 %
#     pixel-missing ones.
# A pixel-missing Gaussian: scale 0.2 px (sigma^2 = 0.04 + 0.3 = 0.34 px^2), centred on a half-pixel position at least 1.5 px inside
# a quadrant, opacity 0.006: 2 ln(255 x 0.006) = 0.85 > 0 = the box minimum, so the reach bit of its quadrant is set, while the nearest
# pixel centres are at d^2 = 0.5: q = 0.5 / 0.34 = 1.47 > 0.85 — no pixel passes the alpha test.
N_FRONT, N_NEAR_PER_QUAD, N_BEHIND = 6, 24, 110


def occluder_scene(C, W=32, H=32, ox=0, oy=0, finished=(0, 1, 2), seed=11):
    n = N_FRONT + N_NEAR_PER_QUAD * len(finished) + N_BEHIND
    sc = make_scene(n, W, H, C, seed, scale_median=0.02)
    g = torch.Generator().manual_seed(seed)
    cam = sc.camera
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    px, py, z, sig, op = (torch.zeros(n) for _ in range(5))

    def half_pixel(m):   # half-pixel positions >= 1.5 px inside a random quadrant of the tile
        q = torch.randint(0, 4, (m,), generator=g)
        cx = ox + 8.0 * (q & 1) + 1.5 + torch.randint(0, 6, (m,), generator=g)
        cy = oy + 8.0 * (q >> 1) + 1.5 + torch.randint(0, 6, (m,), generator=g)
        return cx, cy

    a = 0
    px[a:a + N_FRONT], py[a:a + N_FRONT] = half_pixel(N_FRONT)
    z[a:a + N_FRONT] = 1.0 + 0.01 * torch.arange(N_FRONT)
    sig[a:a + N_FRONT], op[a:a + N_FRONT] = 0.2, 0.006
    a += N_FRONT
    for k, q in enumerate(finished):
        s = slice(a, a + N_NEAR_PER_QUAD)
        i = torch.arange(N_NEAR_PER_QUAD)
        px[s], py[s] = ox + 8.0 * (q & 1) + 1.5 + 4.0 * (i & 1), oy + 8.0 * (q >> 1) + 1.5 + 4.0 * ((i >> 1) & 1)
        z[s] = 1.2 + 0.001 * (i * len(finished) + k)
        sig[s], op[s] = 3.0, 0.99
        a += N_NEAR_PER_QUAD
    s = slice(a, n)
    m = N_BEHIND
    tiny = torch.rand(m, generator=g) < 0.4
    hx, hy = half_pixel(m)
    rx, ry = ox + 0.5 + 15.0 * torch.rand(m, generator=g), oy + 0.5 + 15.0 * torch.rand(m, generator=g)
    px[s], py[s] = torch.where(tiny, hx, rx), torch.where(tiny, hy, ry)
    zz = torch.empty(m)
    zz[torch.randperm(m, generator=g)] = 1.5 + 2.5 * (torch.arange(m, dtype=torch.float32) + 0.5) / m
    z[s] = zz
    sig[s] = torch.where(tiny, torch.tensor(0.2), torch.tensor(0.25))
    op[s] = torch.where(tiny, torch.tensor(0.006), torch.tensor(0.5))
    # (the projection puts camera-space x / z = 0 at pixel (W - 1) / 2 - 0.5: seen in the oracle's xy, asserted by the host test)
    sc.means3D[:, 0] = (px + 0.5 - (W - 1) / 2.0) / fx * z
    sc.means3D[:, 1] = (py + 0.5 - (H - 1) / 2.0) / fy * z
    sc.means3D[:, 2] = z
    sc.scales[:] = (sig * z / fx)[:, None]
    sc.opacities[:, 0] = op
    return sc


SCENES = {
    "occluder": dict(W=32, H=32, ox=0, oy=0, finished=(0, 1, 2)),
    # 40 x 24: of tile (2, 0) only quadrants 0 and 2 have pixels (x < 40), of tile row 1 only quadrants 0 and 1 (y < 24)
    "edge": dict(W=40, H=24, ox=32, oy=0, finished=(0, 1)),
    "edge_row": dict(W=40, H=24, ox=16, oy=16, finished=(0, 3)),
}
