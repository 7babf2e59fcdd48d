"""Generates tests/golden/selection.npz from the reference's OWN utils/selection.py (SplatLoc's landmark selection,
gaussian_selectition, :91-157), imported in THIS container (it needs only numpy and tqdm):

    inside_check                  :27-40   visibility per (point, view)
    Computedist2surfarce          :66-81   mean / population std of the kept |pc.z - depth| per point
    ComputePerPointAngularSpan    :42-64   acos(clip(1 - 2 lmin/lmax, 0, 1)) of the averaged I - b b^T
    gaussian_selectition          :91-157  score, np.argsort, greedy pick at radius 18, 9, 4.5, ...

on a synthetic 8 x 6 x 3 m room seen by cameras inside it.  Depth maps are 480 x 640 but stored as 60 x 80 uint16 millimetre
grids with zero holes; `expand_depths` (restated in the tests) widens them exactly with np.repeat.

Fixture A (~2.5k points, 32 views): points on the walls (offset 3-12 cm along the wall normal, so that every diff is well
above the f32 rounding of the reference's pc.z) and points inside the room, with n_visible 0 (one point: every such point
scores exactly 4), 1 and >= 2, n_depth < n_visible.  Points are dropped when any (point, view) pair lies within 1e-4 px of a
pixel edge or of the image bounds, or within 1e-6 of the z, diff or depth thresholds (f64 restatement below), and when the
reference's f32 depth statistics or span differ from the f64 ones by more than the tests' bars (1e-5 relative; 1e-6
where n_visible >= 2: the reference normalises b in f32, which moves spans of nearly collinear views by up to ~3e-6).  Scores are pairwise
distinct, so the reference's unstable argsort has one answer.  Greedy picks for num_gs in {1, 40, 400}.

Fixture B (256 points, every n_visible >= 2, sorted scores >= 1e-5 apart; seed search): the reference's whole
gaussian_selectition for num_gs = 64, which the drop-in must reproduce exactly.

Only the fixture (data) is committed; nothing of the reference travels.
"""
import io
import os
import sys
import contextlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, CELL = 640, 480, 8
K = np.array([[320.0, 0.0, 319.5], [0.0, 318.0, 239.5], [0.0, 0.0, 1.0]])
ROOM = np.array([8.0, 6.0, 3.0])


def expand_depths(mm):
    """[M, 60, 80] uint16 millimetres -> [M, 480, 640] float32 metres"""
    d = np.repeat(np.repeat(mm, CELL, axis=1), CELL, axis=2)
    return d.astype(np.float32) / np.float32(1000.0)


def look_w2c(c, yaw, pitch):
    fwd = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])            # rows: camera x, y, z in world
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ c
    return T.astype(np.float32)


def render_mm(w2c, rng, holes):
    """z-depth of the room's walls at each 8 x 8 cell centre, in millimetres"""
    R = w2c[:3, :3].astype(np.float64)
    t = w2c[:3, 3].astype(np.float64)
    c = -R.T @ t
    v, u = np.meshgrid(np.arange(H // CELL) * CELL + CELL / 2, np.arange(W // CELL) * CELL + CELL / 2, indexing="ij")
    rays_c = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    rays_w = rays_c @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        t_hi = np.where(rays_w > 0, (ROOM - c) / rays_w, np.inf)
        t_lo = np.where(rays_w < 0, (0.0 - c) / rays_w, np.inf)
    tt = np.minimum(t_hi, t_lo).min(-1)          # z of the camera ray is 1: the ray parameter is the z-depth
    mm = np.round(tt * 1000.0).astype(np.uint16)
    mm[rng.random(mm.shape) < holes] = 0
    return mm


def make_views(rng, M):
    w2cs, mms = [], []
    for _ in range(M):
        c = np.array([rng.uniform(1.5, 6.5), rng.uniform(1.5, 4.5), rng.uniform(1.0, 2.0)])
        w2c = look_w2c(c, rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.2))
        w2cs.append(w2c)
        mms.append(render_mm(w2c, rng, 0.05))
    return np.stack(w2cs), np.stack(mms)


def make_points(rng, n_wall, n_free):
    pts = []
    for _ in range(n_wall):
        ax = rng.integers(0, 3)
        side = rng.integers(0, 2)
        p = rng.uniform([0.2, 0.2, 0.2], ROOM - 0.2)
        off = rng.uniform(0.03, 0.12) * rng.choice([-1.0, 1.0])
        p[ax] = side * ROOM[ax] + (off if side == 0 else -off)
        pts.append(p)
    pts += list(rng.uniform([0.3, 0.3, 0.3], ROOM - 0.3, size=(n_free, 3)))
    return np.array(pts, np.float32)


def restate(points, w2cs, depths):
    """f64 visibility, pixel, kept-diff flags per (point, view) and a 'too close to a decision' flag per point"""
    p = points.astype(np.float64)
    R = w2cs[:, :3, :3].astype(np.float64)
    t = w2cs[:, :3, 3].astype(np.float64)
    pc = np.einsum("mij,nj->nmi", R, p) + t[None]
    q = pc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    front = pc[..., 2] >= 0.01
    vis = front & (u > 0) & (u < W) & (v > 0) & (v < H)
    near = np.abs(pc[..., 2] - 0.01) < 1e-6
    frac = lambda x: np.abs(x - np.round(x))  # noqa: E731
    inb = front & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
    near |= inb & ((frac(u) < 1e-4) | (frac(v) < 1e-4))
    ui = np.clip(np.where(vis, u, 0).astype(np.int64), 0, W - 1)
    vi = np.clip(np.where(vis, v, 0).astype(np.int64), 0, H - 1)
    d = depths[np.arange(len(w2cs))[None, :], vi, ui].astype(np.float64)
    diff = np.abs(pc[..., 2] - d)
    near |= vis & ((np.abs(diff - 0.3) < 1e-6) | (np.abs(d - 0.02) < 1e-6))
    kept = vis & (diff < 0.3) & (d > 0.02)
    n = kept.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(kept, diff, 0).sum(1) / n
        std = np.sqrt(np.where(kept, (diff - mean[:, None]) ** 2, 0).sum(1) / n)
    e = p[:, None, :] - t[None]
    b = np.einsum("mji,nmj->nmi", R, e)
    b /= np.linalg.norm(b, axis=-1, keepdims=True)
    Hm = np.where(vis[..., None, None], np.eye(3) - b[..., :, None] * b[..., None, :], 0.0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ev = np.linalg.eigvalsh(Hm / np.maximum(vis.sum(1), 1)[:, None, None])
        span = np.where(vis.sum(1) > 0, np.arccos(np.clip(1 - 2 * ev[:, 0] / ev[:, 2], 0, 1)), 0.0)
    return vis, kept, near.any(1), mean, std, span


def reference_run(sel, points, w2cs, depths, nums):
    n = len(points)
    nvis = np.zeros(n, np.int32)
    for i in range(n):
        nvis[i] = sum(bool(sel.inside_check(points[i], w2cs[m], K)[0]) for m in range(len(w2cs)))
    mean = np.zeros(n)
    std = np.zeros(n)
    span = np.zeros(n)
    scores = np.zeros(n)
    with warnings_off():
        for i in range(n):
            m, s = sel.Computedist2surfarce(points[i], w2cs, K, depths)
            a = sel.ComputePerPointAngularSpan(points[i], w2cs, K)
            mean[i], std[i], span[i] = m, s, a
            scores[i] = min(2, 0.05 / m) + min(2, 0.05 / s) + a     # gaussian_selectition :111-113, its own scalar types
    picks = {}
    for num in nums:
        with warnings_off(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            picks[num] = sel.gaussian_selectition(points, w2cs, K, depths, num_gs=num)
    return nvis, mean, std, span, scores, picks


@contextlib.contextmanager
def warnings_off():
    import warnings
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def main():
    sys.path.insert(0, "/root/reference")
    from utils import selection as sel

    # ---- fixture A
    rng = np.random.default_rng(20261015)
    w2cs, mm = make_views(rng, 32)
    depths = expand_depths(mm)
    pts = make_points(rng, 2000, 900)
    pts = np.concatenate([pts, np.array([[4.0, 3.0, -5.0]], np.float32)])    # below the floor: behind / outside every view
    vis, kept, near, mean64, std64, span64 = restate(pts, w2cs, depths)
    nvis64 = vis.sum(1)
    keep = ~near
    zero = np.flatnonzero(keep & (nvis64 == 0))
    keep[zero[:-1]] = False                         # one n_visible == 0 point: they all score exactly 4
    # the reference's f32 statistics must sit inside the tests' 1e-5 relative bar of the f64 ones
    sub = np.flatnonzero(keep)
    with warnings_off():
        ref_ms = np.array([sel.Computedist2surfarce(pts[i], w2cs, K, depths) for i in sub], np.float64)
    ok = kept[sub].sum(1) == 0
    ok |= (np.abs(ref_ms[:, 0] - mean64[sub]) <= 1e-5 * np.abs(mean64[sub])) & \
          (np.abs(ref_ms[:, 1] - std64[sub]) <= 1e-5 * np.abs(std64[sub]))
    keep[sub[~ok]] = False
    # ... and so must the reference's span (b normalised in f32) where n_visible >= 2: 1e-6 absolute
    sub = np.flatnonzero(keep & (nvis64 >= 2))
    with warnings_off():
        ref_span = np.array([sel.ComputePerPointAngularSpan(pts[i], w2cs, K) for i in sub], np.float64)
    bad_span = np.abs(ref_span - span64[sub]) > 1e-6
    keep[sub[bad_span]] = False
    print(f"A: {len(pts)} points, {int((~keep).sum())} dropped ({int(near.sum())} near a decision, {int((~ok).sum())} "
          f"by the f32 statistics bar, {int(bad_span.sum())} by the span bar)")
    pa = pts[keep]
    nvis, mean, std, span, scores, _ = reference_run(sel, pa, w2cs, depths, ())
    # n_visible == 1 spans can round to exactly 0 (lmin <= 0 in the reference's f32 b): keep one point of each tied score
    o = np.lexsort((nvis, scores))                  # within a tie the smallest n_visible (the n_visible == 0 point) stays
    uniq = np.zeros(len(pa), bool)
    uniq[o[np.r_[True, scores[o][1:] != scores[o][:-1]]]] = True
    print(f"A: {int((~uniq).sum())} points with a tied score dropped, tied values {np.unique(scores[~uniq])[:5]}")
    keep[np.flatnonzero(keep)[~uniq]] = False
    pa = pts[keep]
    nvis, mean, std, span, scores, picks = reference_run(sel, pa, w2cs, depths, (1, 40, 400))
    ndepth = kept[keep].sum(1).astype(np.int32)
    assert np.array_equal(nvis, nvis64[keep])
    assert len(np.unique(scores)) == len(scores), "fixture A scores must be pairwise distinct"
    assert (nvis == 0).sum() == 1 and (nvis == 1).sum() > 20 and (nvis >= 2).sum() > 500
    assert (ndepth < nvis).sum() > 100
    behind = np.einsum("mij,nj->nmi", w2cs[:, :3, :3].astype(np.float64), pa.astype(np.float64))[..., 2] + w2cs[:, 2, 3] < 0
    assert behind.any(1).sum() > 500
    # the pick for 400 needs >= 4 halvings of the radius: its last landmark is closer than 18/16 to an earlier one
    p400 = picks[400]
    dmin = min(np.linalg.norm(p400[:k] - p400[k], axis=1).min() for k in range(1, 400))
    assert dmin < 18.0 / 16, dmin
    print(f"A: {len(pa)} points, n_visible 0/1/>=2 = {(nvis == 0).sum()}/{(nvis == 1).sum()}/{(nvis >= 2).sum()}, "
          f"n_depth < n_visible: {(ndepth < nvis).sum()}, smallest distance in the 400-pick {dmin:.3f}")

    # ---- fixture B
    for seed in range(1, 200):
        rb = np.random.default_rng(seed)
        wb, mb = make_views(rb, 24)
        db = expand_depths(mb)
        pb = make_points(rb, 300, 200)
        vb, _, nb_near, _, _, _ = restate(pb, wb, db)
        good = (~nb_near) & (vb.sum(1) >= 2)
        if good.sum() < 256:
            continue
        pb = pb[np.flatnonzero(good)[:256]]
        vb, _, _, _, _, _ = restate(pb, wb, db)
        with warnings_off():
            sb = np.array([min(2, 0.05 / m) + min(2, 0.05 / s) + sel.ComputePerPointAngularSpan(p, wb, K)
                           for p in pb for (m, s) in [sel.Computedist2surfarce(p, wb, K, db)]])
        if np.diff(np.sort(sb)).min() >= 1e-5:
            break
    else:
        raise RuntimeError("no seed gives fixture B sorted scores 1e-5 apart")
    with warnings_off(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        pick_b = sel.gaussian_selectition(pb, wb, K, db, num_gs=64)
    print(f"B: seed {seed}, min score gap {np.diff(np.sort(sb)).min():.2e}")

    np.savez_compressed(
        os.path.join(HERE, "selection.npz"),
        K=K, a_points=pa, a_w2cs=w2cs, a_depth_mm=mm, a_n_visible=nvis, a_n_depth=ndepth, a_depth_mean=mean,
        a_depth_std=std, a_span=span, a_score=scores, a_pick_1=picks[1], a_pick_40=picks[40], a_pick_400=picks[400],
        b_points=pb, b_w2cs=wb, b_depth_mm=mb, b_score=sb, b_pick_64=pick_b)


if __name__ == "__main__":
    main()
