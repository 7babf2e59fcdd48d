"""Absolute pose on the MI355X (csrc/pnp.hip through splatloc_amd.pnp) against the f64 restatement of tests/test_host_pnp.py
and planted poses: stage by stage (samples, models, scores), whole problems, determinism, batching, degenerate inputs and the
localisation chain frustum candidates -> decoder -> Hungarian matching -> solve_pose."""
import ctypes as C

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import pnp as P
from splatloc_amd.rasterizer import _stream
from tests.test_host_pnp import (REPLICA, SCENE12, hypotheses, planted_scene, pose_errors, residuals, score)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _table(items):
    probs, off = [], 0
    for p2, _, intr in items:
        probs.append(P.PnpProblem(off, len(p2), 0, *intr))
        off += len(p2)
    return (P.PnpProblem * len(items))(*probs)


def _dev(items):
    p2 = torch.from_numpy(np.concatenate([a for a, _, _ in items])).to(DEV)
    p3 = torch.from_numpy(np.concatenate([b for _, b, _ in items])).to(DEV)
    return p2, p3


def _ws(lib, B, tab, opt):
    return torch.empty(int(lib.splatraster_pnp_workspace_bytes(B, tab, C.byref(opt))), dtype=torch.uint8, device=DEV)


def test_hypotheses_match_restatement():
    lib = _native.load()
    items = []
    for k, (n, cam) in enumerate(((7, SCENE12), (300, REPLICA), (4096, SCENE12))):
        p2, p3, *_rest = planted_scene(40 + k, n, 0.3 if n > 7 else 0.0, cam)
        items.append((p2, p3, _rest[3]))
    opt = P.options(seed=77)
    tab = _table(items)
    p2, p3 = _dev(items)
    T, trial0 = 256, 3000
    B = len(items)
    samples = torch.empty((B, T, 3), dtype=torch.int32, device=DEV)
    models = torch.zeros((B, T, 4, 12), dtype=torch.float64, device=DEV)
    nmod = torch.empty((B, T), dtype=torch.int32, device=DEV)
    ws = _ws(lib, B, tab, opt)
    st = lib.splatraster_pnp_hypotheses(B, tab, C.byref(opt), trial0, T, P._ptr(p2), P._ptr(p3), P._ptr(samples),
                                        P._ptr(models), P._ptr(nmod), P._ptr(ws), _stream(DEV))
    assert st == 0
    s, m, nm = samples.cpu().numpy(), models.cpu().numpy(), nmod.cpu().numpy()
    total = 0
    for b, (a2, a3, intr) in enumerate(items):
        for k in range(T):
            idx, ms = hypotheses(a2, a3, intr, 77, trial0 + k)
            assert tuple(s[b, k]) == idx, (b, k)
            assert nm[b, k] == len(ms), (b, k)
            for q, want in enumerate(ms):
                want = np.array(want)
                assert np.abs(m[b, k, q] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (b, k, q)
            total += len(ms)
    assert total > B * T


def test_scores_match_restatement():
    lib = _native.load()
    items, mods = [], []
    rng = np.random.default_rng(5)
    for k, n in enumerate((50, 1000, 4096)):
        p2, p3, R, t, _, intr, _ = planted_scene(60 + k, n, 0.5, SCENE12)
        items.append((p2, p3, intr))
        cand = [np.concatenate([R.reshape(-1), t])]
        for _ in range(15):   # perturbed models: residuals spread over the threshold
            w = rng.normal(size=3) * 0.01
            from tests.test_host_pnp import expso3
            cand.append(np.concatenate([(expso3(w) @ R).reshape(-1), t + rng.normal(size=3) * 0.02]))
        mods.append(np.stack(cand))
    M = 16
    opt = P.options(max_error_px=12.0)
    tab = _table(items)
    p2, p3 = _dev(items)
    md = torch.from_numpy(np.stack(mods)).to(DEV).contiguous()
    cnt = torch.empty((len(items), M), dtype=torch.int32, device=DEV)
    sm = torch.empty((len(items), M), dtype=torch.float64, device=DEV)
    ws = _ws(lib, len(items), tab, opt)
    assert lib.splatraster_pnp_score(len(items), tab, C.byref(opt), M, P._ptr(md), P._ptr(p2), P._ptr(p3), P._ptr(cnt),
                                     P._ptr(sm), P._ptr(ws), _stream(DEV)) == 0
    c, s = cnt.cpu().numpy(), sm.cpu().numpy()
    for b, (a2, a3, intr) in enumerate(items):
        for q in range(M):
            r, _ = residuals(mods[b][q], a2, a3, intr)
            if np.any(np.abs(r - 144.0) <= 1e-9 * 144.0):
                continue   # a residual on the threshold: the count may differ by rounding
            wc, wsum = score(mods[b][q], a2, a3, intr, 12.0)
            assert c[b, q] == wc, (b, q)
            assert abs(s[b, q] - wsum) <= 1e-9 * max(1.0, wsum), (b, q)


CASES = [(n, share) for n in (4, 6, 50, 500, 4096) for share in (0.0, 0.3, 0.6, 0.8)
         if n * (1 - share) >= 20 or (n <= 6 and share == 0.0)]


@pytest.mark.parametrize("camera", [REPLICA, SCENE12], ids=["replica", "scene12"])
@pytest.mark.parametrize("n,share", CASES)
def test_planted_scenes(camera, n, share):
    p2, p3, R0, t0, inl, intr, depth = planted_scene(1000 + n + int(share * 10), n, share, camera)
    ret = P.absolute_pose_estimation(p2, p3, camera)
    assert ret["success"]
    R = P.qvec_to_rotmat(ret["qvec"])
    dr, dt = pose_errors(R, ret["tvec"], R0, t0)
    assert dr < 0.05 and dt < 1e-3 * depth, (dr, dt, depth)
    r, _ = residuals(np.concatenate([R0.reshape(-1), t0]), p2, p3, intr)
    assert ret["inliers"].dtype == np.bool_ and ret["inliers"].shape == (n,)
    assert ret["inliers"][inl & (r < 121.0)].all()
    assert not ret["inliers"][~inl & (r > 169.0)].any()
    assert ret["num_inliers"] == int(ret["inliers"].sum())
    q = ret["qvec"]
    assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-12
    # solve_pose's c2w is the inverse of the refined world-to-camera pose
    Rc, tc, ret2 = P.solve_pose(p2.astype(np.float32), p3.astype(np.float32), camera)
    if ret2["success"]:
        dr2, dt2 = pose_errors(Rc, tc, R0.T, -R0.T @ t0)
        assert dr2 < 0.05 and dt2 < 1e-3 * depth + 1e-3


def _bits(r):
    return [x.cpu().numpy().tobytes() for x in (r["R"], r["t"], r["inliers"], r["num_inliers"], r["success"], r["trials"])]


def test_deterministic_and_batch_equals_single():
    probs = []
    for k, (n, share) in enumerate(((50, 0.3), (500, 0.6), (4096, 0.3), (6, 0.0), (3, 0.0), (1000, 0.8))):
        if n < 4:
            probs.append((np.zeros((n, 2)), np.zeros((n, 3)), np.eye(3)))
            continue
        p2, p3, _, _, _, intr, _ = planted_scene(2000 + k, n, share, SCENE12 if k % 2 else REPLICA)
        fx, fy, cx, cy = intr
        probs.append((torch.from_numpy(p2).to(DEV), p3.astype(np.float64), np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])))
    single = [P.estimate_absolute_pose(*p, seed=11) for p in probs]
    again = [P.estimate_absolute_pose(*p, seed=11) for p in probs]
    batch = P.estimate_absolute_pose_batch(probs, seed=11)
    for a, b, c in zip(single, again, batch):
        assert _bits(a) == _bits(b) == _bits(c)
    assert not bool(single[4]["success"]) and int(single[4]["trials"]) == 0
    assert all(bool(single[i]["success"]) for i in (0, 1, 2, 3, 5))
    assert single[0]["R"].device.type == "cuda" and single[0]["inliers"].dtype == torch.bool


def test_degenerate_inputs_fail_without_nan():
    cam = SCENE12
    assert P.absolute_pose_estimation(np.zeros((3, 2)), np.zeros((3, 3)), cam) == {"success": False}
    rng = np.random.default_rng(8)
    s = rng.uniform(0, 1, size=(200, 1))
    line = np.array([0.0, 0.0, 3.0]) + s * np.array([1.0, 0.5, 0.2])
    uv = rng.uniform(0, 640, size=(200, 2))
    assert P.absolute_pose_estimation(uv, line, cam) == {"success": False}
    same = np.tile(np.array([[0.3, 0.2, 4.0]]), (100, 1))
    assert P.absolute_pose_estimation(uv[:100], same, cam) == {"success": False}
    K = np.array([[572.0, 0, 320], [0, 572.0, 240], [0, 0, 1]])
    for p2, p3 in ((uv, line), (uv[:100], same)):
        r = P.estimate_absolute_pose(p2, p3, K, max_num_trials=2000)
        assert not bool(r["success"]) and bool(torch.isfinite(r["R"]).all()) and bool(torch.isfinite(r["t"]).all())


def test_full_localisation_chain():
    """a synthetic room: frustum candidates of the database frame (subset mode), a lookup decoder, Hungarian matching of
    planted query descriptors (with distractors) and solve_pose recover the query's camera-to-world pose"""
    from splatloc_amd import matching as Mt
    from tests.golden.make_golden_matching import look_at, wall_points
    rng = np.random.default_rng(21)
    W, H = 640, 480
    K = np.array([[572.0, 0, 320], [0, 572.0, 240], [0, 0, 1]])
    pts = wall_points(rng, 3000)
    db_c2w = look_at(np.array([1.5, 1.2, 1.4]), np.array([5.5, 4.0, 1.2]))
    q_c2w = look_at(np.array([1.6, 1.15, 1.45]), np.array([5.4, 4.1, 1.25]))
    D = 64
    feats = rng.standard_normal((len(pts), D)).astype(np.float32)
    lut = {tuple(p): f for p, f in zip(np.asarray(pts, np.float64).tolist(), feats)}
    decoder = lambda x: torch.from_numpy(np.stack([lut[tuple(p)] for p in x.double().numpy().tolist()]))  # noqa: E731
    frame = {"w2c": torch.from_numpy(np.linalg.inv(db_c2w)), "c2w": torch.from_numpy(db_c2w)}
    p3d, f3d, _ = Mt.get_frusm_pts(None, None, frame, K, W, H, decoder=decoder, subset=pts)
    assert len(p3d) > 200
    # query keypoints: projections of a share of the candidates into the query view, plus distractors
    w2c = np.linalg.inv(q_c2w)
    pc = p3d @ w2c[:3, :3].T + w2c[:3, 3]
    uv = pc[:, :2] / pc[:, 2:] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    vis = np.flatnonzero((pc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H))
    sel = rng.choice(vis, size=min(len(vis), 300), replace=False)
    q_kps = uv[sel] + rng.normal(size=(len(sel), 2)) * 0.5
    q_desc = f3d.numpy()[sel] + rng.normal(size=(len(sel), D)).astype(np.float32) * 0.3
    n_distract = 60
    q_kps = np.concatenate([q_kps, rng.uniform(0, [W, H], size=(n_distract, 2))])
    q_desc = np.concatenate([q_desc, rng.standard_normal((n_distract, D)).astype(np.float32)])
    out = Mt.HungarianMatcher()({"query_descs": torch.from_numpy(q_desc.T.copy()), "train_descs": f3d.T})
    m = out["matches"].numpy()
    r, t, ret = P.solve_pose(q_kps[m[0]], p3d[m[1]], {"model": "OPENCV", "width": W, "height": H,
                                                      "params": [572.0, 572.0, 320.0, 240.0, 0., 0., 0., 0.]})
    assert ret["success"]
    depth = float(np.median(pc[sel, 2]))
    dr, dt = pose_errors(r, t, q_c2w[:3, :3], q_c2w[:3, 3])
    assert dr < 0.05 and dt < 1e-3 * depth, (dr, dt)
