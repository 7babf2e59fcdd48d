"""Test-side restatements for the 2D-3D matching (splatloc_amd/matching.py, csrc/matching.hip), beside fusion_reference.py and
decoder_reference.py:

    frustum_restated  the frustum candidates of INTEGRATION.md §17 in float64 numpy, element by element in the documented
                      operation order (no BLAS, no np.dot), with a brute-force nearest neighbour: an exact oracle for
                      fr_point_kernel / fr_query_kernel, ties and decision edges included
    cost_f64          the descriptor similarity and the thresholded cost in float64
    cost_bound        the derived f32 error bound of one device similarity
    room_scene / grid_scene / with_duplicates / cost_cases
                      the synthetic inputs the host and the device tests share (elementwise numpy on default_rng draws)

Nothing here imports the product."""
import numpy as np

from tests.golden.make_golden_matching import descriptors, look_at

Z_NEAR = 0.05
NN_RADIUS = 0.1
FAR = 1e15            # a back-projection at or beyond this magnitude (or non-finite) yields no pair
CHUNK_ELEMENTS = 1 << 22


def _affine(m, x, y, z):
    """rows of the 3 x 4 transform [R | t] applied as ((r0*x + r1*y) + r2*z) + t, the device's association"""
    return tuple(((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3))


def project(points, w2c, K):
    """(pz, u, v) of the f32-widened points, float64 elementwise"""
    p = np.asarray(points).astype(np.float32).astype(np.float64).reshape(-1, 3)
    m = np.asarray(w2c).astype(np.float64)
    k = np.asarray(K).astype(np.float64)
    px, py, pz = _affine(m, p[:, 0], p[:, 1], p[:, 2])
    q = [(k[r, 0] * px + k[r, 1] * py) + k[r, 2] * pz for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return pz, q[0] / q[2], q[1] / q[2]


def backproject(kp_mask, depth, c2w, kp_K):
    """world positions [n, 3] of the kp_mask == 1 pixels in row-major order and which of them may be searched"""
    rr, cc = np.nonzero(np.asarray(kp_mask) == 1)
    d = np.asarray(depth).astype(np.float32).astype(np.float64)[rr, cc]
    k = np.asarray(kp_K).astype(np.float64)
    m = np.asarray(c2w).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = (cc.astype(np.float64) - k[0, 2]) * d / k[0, 0]
        ys = (rr.astype(np.float64) - k[1, 2]) * d / k[1, 1]
        q = np.stack(_affine(m, xs, ys, d), axis=-1) if len(d) else np.zeros((0, 3))
        ok = (np.isfinite(q) & (np.abs(q) < FAR)).all(axis=1)
    return q, ok


def nearest(kept_xyz, q):
    """brute force: (distance, position in kept_xyz) of the nearest row per query; ties go to the smaller position"""
    n, m = len(q), len(kept_xyz)
    best_d, best_i = np.full(n, np.inf), np.full(n, -1, np.int64)
    if n == 0 or m == 0:
        return best_d, best_i
    step = max(1, CHUNK_ELEMENTS // m)
    for a in range(0, n, step):
        b = min(n, a + step)
        ex = kept_xyz[None, :, 0] - q[a:b, None, 0]
        ey = kept_xyz[None, :, 1] - q[a:b, None, 1]
        ez = kept_xyz[None, :, 2] - q[a:b, None, 2]
        dd = np.sqrt((ex * ex + ey * ey) + ez * ez)
        i = dd.argmin(axis=1)   # the first minimum: kept_xyz is in index order
        best_i[a:b] = i
        best_d[a:b] = dd[np.arange(b - a), i]
    return best_d, best_i


def frustum_restated(points, w2c, K, W, H, marker=None, kp_mask=None, depth=None, c2w=None, kp_K=None,
                     marker_threshold=0.005, return_distance=False):
    """(idx int64 [n], xyz f32 [n, 3], uv f64 [n, 2]) of splatloc_amd.matching.frustum_candidates, INTEGRATION.md §17:
    pc = ((r0*x + r1*y) + r2*z) + t on the f32 points widened to f64, q = (k0*px + k1*py) + k2*pz, u = q0 / q2, v = q1 / q2;
    kept iff pz > 0.05, 0 <= u < W, 0 <= v < H and, in key mode, marker > threshold compared in f32.  Subset mode (marker
    None) returns the kept points in index order.  Key mode pairs every kp_mask == 1 pixel (row-major) with its nearest kept
    point (ties: the smaller index) when sqrt((ex*ex + ey*ey) + ez*ez) < 0.1; a pixel whose back-projection is non-finite
    or >= 1e15 in magnitude gives no pair."""
    pts32 = np.asarray(points).astype(np.float32).reshape(-1, 3)
    pz, u, v = project(pts32, w2c, K)
    with np.errstate(invalid="ignore"):
        keep = (pz > Z_NEAR) & (0.0 <= u) & (u < float(W)) & (0.0 <= v) & (v < float(H))
    uv = np.stack([u, v], axis=-1)
    if marker is None:
        idx = np.flatnonzero(keep)
        return idx, pts32[idx], uv[idx]
    keep &= np.asarray(marker).reshape(-1).astype(np.float32) > np.float32(marker_threshold)
    kept = np.flatnonzero(keep)
    q, ok = backproject(kp_mask, depth, c2w, kp_K)
    dist, pos = nearest(pts32[kept].astype(np.float64), np.where(ok[:, None], q, 0.0))
    found = ok & (dist < NN_RADIUS)
    idx = kept[pos[found]]
    out = (idx, pts32[idx], uv[idx])
    return out + (dist[found],) if return_distance else out


# ---- descriptor cost ------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24   # unit roundoff of float32


def cost_f64(d1, d2, thr):
    """(sim, cost) of match_cost in float64, in the solver's orientation (rows = the smaller set, d1 on a tie): the cosine
    similarity of the columns of d1 [D, N1] and d2 [D, N2] with F.normalize's denominator max(||x||, 1e-12), before the
    threshold, and cost = 1 - where(sim < thr, 0, sim) with thr the f32 value the device compares with"""
    a = d1.astype(np.float64) / np.maximum(np.linalg.norm(d1.astype(np.float64), axis=0), 1e-12)
    b = d2.astype(np.float64) / np.maximum(np.linalg.norm(d2.astype(np.float64), axis=0), 1e-12)
    sim = a.T @ b
    if d2.shape[1] < d1.shape[1]:
        sim = np.ascontiguousarray(sim.T)
    return sim, 1.0 - np.where(sim < float(np.float32(thr)), 0.0, sim)


def cost_bound(D):
    """(2 D + 8) * 2^-24: how far one f32 entry of match_cost_kernel may lie from the f64 value, with u = 2^-24.
    The squared norm is an FMA chain of D non-negative terms: relative error <= D u.  The square root halves that and adds
    u, the division by the norm adds u: a normalised element carries (D / 2 + 2) u, the product of two (D + 4) u.  Summed over
    the D terms that is (D + 4) u * sum|a_i b_i| <= (D + 4) u by Cauchy-Schwarz (both columns have unit length).  The D-term
    FMA chain of the dot product adds D u * sum|a_i b_i| <= D u.  1 - sim rounds once more in f32: half an ulp of a value
    below 2, u.  Together (2 D + 5) u to first order; the remaining 3 u cover the second-order terms (D^2 u^2 < u up to
    D = 4096).  Derived, not measured: numpy's own f32 evaluation stays below 8e-7 at D = 256 against 3.1e-5."""
    return (2 * D + 8) * U32


COST_DIMS = (1, 15, 16, 17, 33, 256)
COST_SHAPES = ((1, 1), (1, 9), (63, 65), (65, 63), (64, 64), (130, 64), (65, 257))
COST_THRESHOLD = 0.4
BAND_SHARE = 1e-3


def cost_cases():
    """(D, N1, N2) of the differential cost tests: every shape in both orientations"""
    shapes = []
    for s in COST_SHAPES:
        for t in (s, s[::-1]):
            if t not in shapes:
                shapes.append(t)
    return [(D, n1, n2) for D in COST_DIMS for n1, n2 in shapes]


def cost_case(D, N1, N2):
    return descriptors(np.random.default_rng(100 + D), D, N1, N2)


def band(sim, thr, D):
    """the entries whose f64 similarity lies within the bound of the threshold: either branch is right there"""
    return np.abs(sim - float(np.float32(thr))) <= cost_bound(D)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def room_scene(seed, N, W, H, density, room=3.0):
    """A key-mode input built from the keypoints outward, in a room centred on the origin (coordinates of both signs): pose,
    intrinsics, mask and f32 depth first; then f32 points at offsets around the 0.1 m bound from the back-projected keypoints
    (lengths in 0.01..0.099 and 0.101..0.2, so both outcomes of d < 0.1 and nearest points in neighbouring grid cells are
    common), background points up to N, all in random order."""
    rng = np.random.default_rng(seed)
    eye = rng.uniform(-0.5, 0.5, 3)
    target = eye + _unit(rng, 1)[0] * np.array([1.0, 1.0, 0.3])
    c2w = look_at(eye, target)
    w2c = np.linalg.inv(c2w)
    f = 0.6 * max(W, H, 2)
    K = np.array([[f, 0.0, (W - 1) / 2], [0.0, f, (H - 1) / 2], [0.0, 0.0, 1.0]])
    mask = (rng.random((H, W)) < density).astype(np.int32)
    depth = rng.uniform(0.5, 3.0, (H, W)).astype(np.float32)
    q, _ = backproject(mask, depth, c2w, K)
    near = np.zeros((0, 3))
    if len(q) and N:
        pick = rng.permutation(np.repeat(np.arange(len(q)), 2))[: max(1, min(2 * len(q), (N * 3) // 4))]
        ln = np.where(rng.random(len(pick)) < 0.5, rng.uniform(0.01, 0.099, len(pick)), rng.uniform(0.101, 0.2, len(pick)))
        near = q[pick] + _unit(rng, len(pick)) * ln[:, None]
    back = rng.uniform(-room, room, (max(N - len(near), 0), 3))
    pts = np.concatenate([near, back])[:N]
    pts = pts[rng.permutation(len(pts))].astype(np.float32).reshape(-1, 3)
    marker = rng.uniform(0.0, 0.02, N).astype(np.float32)
    return dict(points=pts, marker=marker, w2c=w2c, c2w=c2w, K=K, W=W, H=H, mask=mask, depth=depth)


def grid_scene(seed, N, W=17, H=9):
    """Cell boundaries: identity pose, power-of-two intrinsics and depths, so the keypoints back-project onto multiples of
    1/16 of both signs (every other one onto a multiple of the 0.125 m grid cell); points sit on keypoints and at
    offsets that are multiples of 1/32 (exact, equal distances between different points), the rest is a background snapped to
    multiples of 0.125."""
    rng = np.random.default_rng(seed)
    c2w = np.eye(4)
    K = np.array([[8.0, 0.0, 8.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])
    mask = (rng.random((H, W)) < 0.7).astype(np.int32)
    depth = rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=(H, W))
    q, _ = backproject(mask, depth, c2w, K)
    pick = rng.integers(0, len(q), size=(N * 2) // 3)
    near = q[pick] + rng.integers(-4, 5, size=(len(pick), 3)) / 32.0
    back = np.round(rng.uniform(-3.0, 3.0, (N - len(near), 3)) * 8.0) / 8.0
    back[:, 2] = np.abs(back[:, 2])
    pts = np.concatenate([near, back])
    pts = pts[rng.permutation(N)].astype(np.float32)
    marker = rng.uniform(0.0, 0.02, N).astype(np.float32)
    return dict(points=pts, marker=marker, w2c=np.eye(4), c2w=c2w, K=K, W=W, H=H, mask=mask, depth=depth)


def with_duplicates(scene, seed, share=0.05):
    """copies `share` of the points over later indices and half as many over earlier ones (the markers stay per index)"""
    rng = np.random.default_rng(seed)
    s = dict(scene)
    pts = scene["points"].copy()
    n = len(pts)
    k = max(1, int(n * share))
    src = rng.integers(0, n - 1, size=k)
    pts[src + 1 + (rng.integers(0, n, size=k) % (n - 1 - src))] = pts[src]
    src = rng.integers(1, n, size=max(1, k // 2))
    pts[rng.integers(0, n, size=len(src)) % src] = pts[src]
    s["points"] = pts
    return s


def key_args(s):
    """the keyword arguments of frustum_restated / frustum_candidates after (points, w2c, K, W, H)"""
    return dict(marker=s["marker"], kp_mask=s["mask"], depth=s["depth"], c2w=s["c2w"], kp_K=s["K"])
