"""Generates tests/golden/matching.npz for SplatLoc's per-query 2D-3D matching (test.py:247-378):

    hungarian_solve       utils/match_utils.py:5-21   imported from the reference as it is
    get_frusm_pts         test.py:247-285             extracted with ast and run on a stub LocalizeQuery
    get_ref_keyponts_3d   test.py:287-303             (dataset: height, width, K; gaussians: get_xyz, get_marker;
                                                       an identity decoder)
    linear_sum_assignment scipy.optimize              the solver cases

Hungarian cases (h<k>_*): descriptors [D, N] built so that a share of the pairs correlates; seeds are kept only when every
similarity is >= 1e-5 away from 0.4 and scipy's answer does not change when the similarities are recomputed in f64 and
rounded back to f32 (so the device's own f32 summation order cannot move the assignment).

Frustum cases (f_*): a synthetic 6 x 5 x 3 m room, key Gaussians on its walls (offset up to 15 cm along the normal) and a
camera inside it at 64 x 48 pixels.  The depth of each pixel is the distance to the wall along its ray.  Points within 1e-4
px of an image edge or 1e-6 of the z threshold are dropped, and so are keypoint pixels whose nearest point lies within 1e-7 m
of the 0.1 m bound or whose first and second neighbours are within 1e-7 m of each other (f64 restatement below).  Key mode
stores the reference's (ref_pts_3d, ref_pts_2d) and the point indices they came from; subset mode (s_*) runs the same frame
with subset_xyz = a random f64 subset of the points.

Solver cases: small tie-heavy matrices stored whole (l<k>_*) with scipy's indices, and one (4096, 2000) matrix rebuilt from a
seed by `big_cost` (elementwise numpy on default_rng draws, no BLAS) with only its indices stored.

Only the fixture (data) is committed; nothing of the reference travels.  Run: python tests/golden/make_golden_matching.py
<path of the reference checkout> (or set SPLATLOC_REFERENCE).
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FW, FH = 64, 48
FK = np.array([[40.0, 0.0, 31.5], [0.0, 40.0, 23.5], [0.0, 0.0, 1.0]])
ROOM = np.array([6.0, 5.0, 3.0])
BIG_SEED, BIG_SHAPE = 20261016, (4096, 2000)


def big_cost(seed=BIG_SEED, shape=BIG_SHAPE):
    """a thresholded-similarity-like f64 cost, elementwise from default_rng draws (bit-identical everywhere)"""
    rng = np.random.default_rng(seed)
    s = rng.random(shape) ** 3
    s = np.where(s < 0.4, 0.0, s)
    return 1.0 - s


def tie_heavy(rng, shape, kind):
    """the small solver matrices: integer, two-valued, thresholded, uniform"""
    if kind == 0:
        return rng.integers(0, 4, size=shape).astype(np.float64)
    if kind == 1:
        return np.where(rng.random(shape) < 0.5, 1.0, 0.25)
    if kind == 2:
        s = rng.random(shape).astype(np.float32)
        s[s < 0.6] = 0
        return (1 - s).astype(np.float64)
    return np.full(shape, 0.5)


def descriptors(rng, D, N1, N2):
    d1 = rng.standard_normal((D, N1)).astype(np.float32)
    d2 = rng.standard_normal((D, N2)).astype(np.float32)
    k = min(N1, N2) * 2 // 3
    p1, p2 = rng.permutation(N1)[:k], rng.permutation(N2)[:k]
    w = rng.uniform(0.3, 3.0, size=k).astype(np.float32)
    d2[:, p2] = d1[:, p1] * w + d2[:, p2] * rng.uniform(0.2, 1.2, size=k).astype(np.float32)
    return d1, d2


def hungarian_cases(ms):
    import torch
    from scipy.optimize import linear_sum_assignment
    out = {}
    shapes = [(256, 40, 25), (256, 25, 40), (256, 48, 48), (64, 1, 7), (64, 7, 1), (64, 120, 300), (32, 200, 90)]
    seed = 0
    for k, (D, N1, N2) in enumerate(shapes):
        while True:
            seed += 1
            rng = np.random.default_rng(seed)
            d1, d2 = descriptors(rng, D, N1, N2)
            a = torch.nn.functional.normalize(torch.from_numpy(d1), p=2, dim=0)
            b = torch.nn.functional.normalize(torch.from_numpy(d2), p=2, dim=0)
            sim = (a.t() @ b).numpy()
            if np.abs(sim.astype(np.float64) - 0.4).min() < 1e-5:
                continue
            s64 = (a.double().t() @ b.double()).numpy().astype(np.float32)
            s64[s64 < 0.4] = 0
            r2, c2 = linear_sum_assignment(1 - s64)
            m, s = ms.hungarian_solve(torch.from_numpy(d1), torch.from_numpy(d2))
            m = m.numpy()
            if not (np.array_equal(m[0], r2) and np.array_equal(m[1], c2)):
                continue
            break
        out.update({f"h{k}_d1": d1, f"h{k}_d2": d2, f"h{k}_matches": m.astype(np.int64), f"h{k}_sims": s.numpy()})
    out["h_count"] = np.int64(len(shapes))
    return out


def solver_cases():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(7)
    out = {}
    mats = [np.array([[3.0]]), np.array([[4.0, 1.0, 3.0, 2.0, 1.0]]), np.array([[4.0], [1.0], [1.0], [2.0]]),
            np.full((6, 6), 2.0), np.full((5, 9), 1.0), np.full((9, 5), 1.0)]
    mx = [False] * len(mats)
    for kind in range(4):
        for shape in ((7, 7), (5, 11), (11, 5), (30, 70), (70, 30)):
            for maximize in (False, True):
                mats.append(tie_heavy(rng, shape, kind))
                mx.append(maximize)
    # +inf entries that leave a finite assignment
    c = tie_heavy(rng, (8, 12), 0)
    c[rng.random(c.shape) < 0.3] = np.inf
    mats.append(c)
    mx.append(False)
    c = tie_heavy(rng, (12, 8), 2)
    c[3, :] = np.inf   # a whole row of a tall matrix: it stays unassigned
    mats.append(c)
    mx.append(False)
    for k, (c, m) in enumerate(zip(mats, mx)):
        r, cc = linear_sum_assignment(c, maximize=m)
        out.update({f"l{k}_cost": c, f"l{k}_max": np.bool_(m), f"l{k}_rows": r.astype(np.int64), f"l{k}_cols": cc.astype(np.int64)})
    out["l_count"] = np.int64(len(mats))
    r, cc = linear_sum_assignment(big_cost())
    out.update({"big_seed": np.int64(BIG_SEED), "big_shape": np.array(BIG_SHAPE, np.int64), "big_rows": r.astype(np.int64),
                "big_cols": cc.astype(np.int64)})
    return out


def look_at(eye, target):
    f = target - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([0.0, 0.0, 1.0]))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return c2w


def wall_points(rng, n):
    """points on the six faces of the room, pushed off by up to 15 cm along the inward normal"""
    face = rng.integers(0, 6, size=n)
    p = rng.random((n, 3)) * ROOM
    ax, hi = face % 3, face >= 3
    p[np.arange(n), ax] = np.where(hi, ROOM[ax], 0.0)
    off = rng.uniform(-0.02, 0.15, size=n)
    p[np.arange(n), ax] += np.where(hi, -off, off)
    return p


def ray_depth(c2w, K, W, H):
    """z-depth of the room's walls per pixel (f64)"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)   # camera rays, z = 1
    dw = d @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dw > 0, (ROOM - o) / dw, -o / dw)
    return np.nanmin(np.where(t > 0, t, np.inf), axis=-1)


def stub_class(ref):
    """LocalizeQuery's two methods extracted from the reference's test.py, bound to a stub object"""
    src = open(os.path.join(ref, "test.py")).read()
    tree = ast.parse(src)
    fns = [n for c in ast.walk(tree) if isinstance(c, ast.ClassDef) for n in c.body
           if isinstance(n, ast.FunctionDef) and n.name in ("get_frusm_pts", "get_ref_keyponts_3d")]
    assert len(fns) == 2
    import torch
    from scipy.spatial import cKDTree
    ns = {"np": np, "torch": torch, "cKDTree": cKDTree}
    mod = ast.Module(body=[ast.ClassDef(name="Stub", bases=[], keywords=[], body=fns, decorator_list=[])], type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), "test.py", "exec"), ns)
    return ns["Stub"]


def frustum_cases(ref):
    import torch
    Stub = stub_class(ref)
    rng = np.random.default_rng(11)
    pts = wall_points(rng, 12000).astype(np.float32)
    marker = rng.uniform(0.0, 0.02, size=(len(pts), 1)).astype(np.float32)
    c2w = look_at(np.array([1.5, 1.2, 1.4]), np.array([5.5, 4.0, 1.2])).astype(np.float32)
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    depth = ray_depth(c2w.astype(np.float64), FK, FW, FH).astype(np.float32)
    mask = (rng.random((FH, FW)) < 0.3).astype(np.int32)
    # f64 restatement: drop points on a decision edge
    P = pts.astype(np.float64)
    pc = P @ w2c[:3, :3].astype(np.float64).T + w2c[:3, 3].astype(np.float64)
    q = pc @ FK.T
    u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    edge = (np.abs(pc[:, 2] - 0.05) < 1e-6) | (np.abs(u) < 1e-4) | (np.abs(u - FW) < 1e-4) | (np.abs(v) < 1e-4) | \
           (np.abs(v - FH) < 1e-4)
    pts, marker = pts[~edge], marker[~edge]
    P = pts.astype(np.float64)
    keep = (pc[~edge, 2] > 0.05) & (u[~edge] >= 0) & (u[~edge] < FW) & (v[~edge] >= 0) & (v[~edge] < FH) & \
           (marker[:, 0] > np.float32(0.005))
    # ... and keypoint pixels whose nearest-neighbour decision is on an edge
    rr, cc = np.nonzero(mask == 1)
    d = depth[rr, cc].astype(np.float64)
    xc = np.stack([(cc - FK[0, 2]) * d / FK[0, 0], (rr - FK[1, 2]) * d / FK[1, 1], d], -1)
    kw = xc @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3].astype(np.float64)
    kept = P[keep]
    for k in range(len(kw)):
        dist = np.sort(np.sqrt(((kept - kw[k]) ** 2).sum(1)))
        if abs(dist[0] - 0.1) < 1e-7 or (len(dist) > 1 and dist[1] - dist[0] < 1e-7):
            mask[rr[k], cc[k]] = 0

    class Dataset:
        height, width, K = FH, FW, FK

    class Gaussians:
        get_xyz = torch.from_numpy(pts)
        get_marker = torch.from_numpy(marker)

    frame = {"K": FK, "c2w": torch.from_numpy(c2w), "w2c": torch.from_numpy(w2c), "depth": torch.from_numpy(depth),
             "sp_kp_mask": torch.from_numpy(mask)}
    s = Stub()
    s.train_dataset, s.gaussians, s.sp_kp_thre, s.feat_decoder = Dataset(), Gaussians(), 0.005, (lambda x: x)
    s.subset_xyz = None
    p3, f3, p2 = s.get_frusm_pts(frame)
    lut = {tuple(r): i for i, r in enumerate(pts.tolist())}
    assert len(lut) == len(pts)
    idx = np.array([lut[tuple(r)] for r in p3.tolist()], np.int64)
    out = {"f_points": pts, "f_marker": marker, "f_w2c": w2c, "f_c2w": c2w, "f_K": FK, "f_depth": depth, "f_mask": mask,
           "f_size": np.array([FW, FH], np.int64), "f_idx": idx, "f_pts3d": p3, "f_pts2d": p2}
    # subset mode: a random f64 subset of the (f32) points
    sub = pts[np.sort(rng.choice(len(pts), 3000, replace=False))].astype(np.float64)
    s.subset_xyz = sub
    q3, _, q2 = s.get_frusm_pts(frame)
    lut = {tuple(r): i for i, r in enumerate(sub.tolist())}
    out.update({"s_subset": sub, "s_idx": np.array([lut[tuple(r)] for r in q3.tolist()], np.int64), "s_pts3d": q3,
                "s_pts2d": q2})
    print("frustum: %d key pairs (%d distinct points, %d keypoints), %d subset points" %
          (len(idx), len(np.unique(idx)), int(mask.sum()), len(q3)))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    sys.path.insert(0, ref)
    from utils import match_utils as ms
    out = {}
    out.update(hungarian_cases(ms))
    out.update(solver_cases())
    out.update(frustum_cases(ref))
    path = os.path.join(HERE, "matching.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
