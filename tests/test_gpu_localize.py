"""Device localisation (splatloc_amd/localize.py, csrc/retrieval.hip) against the reference fixture tests/golden/localize.npz,
the numpy restatement tests/localize_reference.py, and — for the batched driver — the stage-by-stage path of INTEGRATION.md
§17 and §18 run per query (matching.get_frusm_pts, HungarianMatcher, pnp.solve_pose), which earlier fixtures pin.

The driver test compares t_c2w bit for bit with solve_pose's `-R^T @ t`, a numpy product: the kernel rounds it as a three-term
FMA chain in ascending order, which is what numpy's BLAS does for this shape on the machines the project is tested on."""
import os

import numpy as np
import pytest
import torch

from splatloc_amd import localize as L
from splatloc_amd import matching as M
from splatloc_amd import pnp as P
from tests import localize_reference as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "localize.npz")
CASES = sorted(LR.RETRIEVAL_CASES)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _norms(x):
    return np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))


@pytest.mark.parametrize("case", CASES)
def test_retrieval_matches_the_reference(golden, case):
    q, db, k, _ = LR.retrieval_case(case)
    assert LR.case_hash(q, db) == str(golden[f"r{case}_sha256"])
    idx, sims = L.retrieve(q, db, k=k)
    assert idx.is_cuda and idx.dtype == torch.int64 and sims.dtype == torch.float32 and tuple(idx.shape) == (q.shape[0], k)
    idx, sims = idx.cpu().numpy(), sims.cpu().numpy()
    assert np.array_equal(idx, golden[f"r{case}_ind"])
    _, s64 = LR.retrieval_topk(q, db, k)
    bound = LR.gamma(q.shape[1]) * _norms(q)[:, None] * _norms(db)[idx]
    err = np.abs(sims.astype(np.float64) - s64)
    print(f"case {case}: max |sims - f64| / bound = {float((err / bound).max()):.4f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("case", sorted(LR.EDGE_CASES))
def test_retrieval_at_the_edges_of_the_shared_staging(case):
    """Q = 33, N = 129 (a row tail of either operand) with D = 36 and D = 33: the oracle's indices (pinned by the cases' margin),
    the similarities within the bound of the cases above; then the same numbers through views one float into their buffers, which
    only the scalar loads can read: idx and sims bit for bit, D = 36 taking the float4 loads from its aligned buffers."""
    q, db, k, _ = LR.retrieval_case(case)
    assert (q.shape, db.shape) == ((33, db.shape[1]), (129, db.shape[1]))
    i64, s64 = LR.retrieval_topk(q, db, k)
    qd, dd = torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda()
    assert qd.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
    idx, sims = L.retrieve(qd, dd, k=k)
    assert np.array_equal(idx.cpu().numpy(), i64)
    bound = LR.gamma(q.shape[1]) * _norms(q)[:, None] * _norms(db)[i64]
    err = np.abs(sims.cpu().numpy().astype(np.float64) - s64)
    print(f"case {case}: max |sims - f64| / bound = {float((err / bound).max()):.4f}")
    assert np.all(err <= bound)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    idx1, sims1 = L.retrieve(shifted(qd), shifted(dd), k=k)
    assert torch.equal(idx1, idx) and torch.equal(sims1.view(torch.int32), sims.view(torch.int32))


@pytest.mark.parametrize("which", (0, 1))
def test_exact_cases_pin_the_tie_rule(which):
    q, db, k, idx_ref, sims_ref = LR.exact_case(which)
    idx, sims = L.retrieve(torch.from_numpy(q), torch.from_numpy(db).cuda(), k=k)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(sims.cpu().numpy(), sims_ref)


@pytest.mark.parametrize("which", (0, 1))
def test_wide_tile_path_is_exact_too(which):
    """problems that fill the chip with 128-query tiles take the kernel's other instantiation (and 64 database slices)"""
    q, db, k, idx_ref, sims_ref = LR.wide_case(which)
    idx, sims = L.retrieve(q, db, k=k)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(sims.cpu().numpy(), sims_ref)
    bad = db.copy()
    bad[-1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        L.retrieve(q, bad, k=k)


def test_retrieval_nan_dtypes_and_a_side_stream(golden):
    q, db, k, _ = LR.retrieval_case(3)
    bad = db.copy()
    bad[200, 7] = np.nan
    with pytest.raises(ValueError, match="descriptors contain non-finite entries"):
        L.retrieve(q, bad, k=k)
    ref = L.retrieve(q, db, k=k)          # the next call starts from a clean status
    assert np.array_equal(ref[0].cpu().numpy(), golden["r3_ind"])
    qh, dh = torch.from_numpy(q).half(), torch.from_numpy(db).half()
    a, b = L.retrieve(qh, dh, k=k), L.retrieve(qh.float(), dh.float(), k=k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    q4, d4, k4, _ = LR.retrieval_case(4)
    a, b = L.retrieve(q4.astype(np.float64), torch.from_numpy(d4).double(), k=k4), L.retrieve(q4, d4, k=k4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    e = L.retrieve(np.zeros((0, 128), np.float32), d4, k=3)
    assert tuple(e[0].shape) == (0, 3) and tuple(e[1].shape) == (0, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        i1, _ = L.retrieve(q, db, k=k)
        i4, _ = L.retrieve(q4, d4, k=k4)
        th, _ = L.pose_errors(golden["p_R_est"], golden["p_t_est"], golden["p_R_gt"], golden["p_t_gt"])
    s.synchronize()
    assert np.array_equal(i1.cpu().numpy(), golden["r3_ind"]) and np.array_equal(i4.cpu().numpy(), golden["r4_ind"])
    assert np.all(np.abs(th.cpu().numpy().astype(np.float64) - golden["p_thetas"].reshape(-1)) <=
                  LR.theta_bound(golden["p_thetas"].reshape(-1).astype(np.float64)))


def test_generate_retrieval_file_writes_the_references_file(golden, tmp_path):
    q, db, k, _ = LR.retrieval_case(1)
    qn = [f"query_{i:04d}.jpg" for i in range(len(q))]
    dn = [f"frame_{i:05d}.jpg" for i in range(len(db))]
    path = tmp_path / "netvlad_retrieval.txt"
    L.generate_retrieval_file(q, db, qn, dn, path, num_matched=k)
    assert open(path, "rb").read() == str(golden["r1_text"]).encode()
    assert L.load_retrieval_results(path)[qn[3]] == [dn[j] for j in golden["r1_ind"][3]]


def test_pose_errors_match_the_reference(golden):
    Re, te, Rg, tg = golden["p_R_est"], golden["p_t_est"], golden["p_R_gt"], golden["p_t_gt"]
    ref_t, ref_d = golden["p_thetas"].reshape(-1).astype(np.float64), golden["p_dists"]
    theta, dist = L.pose_errors(Re, te, torch.from_numpy(Rg).cuda(), tg)
    assert theta.is_cuda and theta.dtype == torch.float32 and dist.dtype == torch.float64
    theta, dist = theta.cpu().numpy(), dist.cpu().numpy()
    err = np.abs(theta.astype(np.float64) - ref_t)
    print("max |theta - ref| / bound =", float((err / LR.theta_bound(ref_t)).max()))
    assert np.all(err <= LR.theta_bound(ref_t))
    assert np.all(np.abs(dist - ref_d) <= 4 * np.spacing(ref_d))
    v = np.ones(len(Re), bool)
    v[[0, 17, 399]] = False
    t2, d2 = L.pose_errors(Re, te, Rg, tg, valid=v)
    t2, d2 = t2.cpu().numpy(), d2.cpu().numpy()
    assert np.isnan(t2[~v]).all() and np.isnan(d2[~v]).all()
    assert np.array_equal(t2[v], theta[v]) and np.array_equal(d2[v], dist[v])
    # the drop-in: the reference's shapes and dtypes, on the host
    T = torch.from_numpy
    thetas, dists = L.eval_pose(T(Re), T(te), T(Rg), T(tg))
    assert not thetas.is_cuda and thetas.dtype == torch.float32 and tuple(thetas.shape) == (len(Re), 1, 1)
    assert not dists.is_cuda and dists.dtype == torch.float64 and tuple(dists.shape) == (len(Re),)
    assert np.array_equal(thetas.numpy().reshape(-1), theta) and np.array_equal(dists.numpy(), dist)
    one_t, one_d = L.eval_pose(T(Re[5:6]), T(te[5:6]), T(Rg[5:6]), T(tg[5:6]))      # test.py's [1, 3, 3] call
    assert tuple(one_t.shape) == (1, 1, 1) and float(one_t) == float(theta[5]) and float(one_d[0]) == float(dist[5])
    # f32 inputs are widened exactly
    f_t, f_d = L.eval_pose(T(Re).float(), T(te).float(), T(Rg).float(), T(tg).float())
    w_t, w_d = L.pose_errors(T(Re).float().double(), T(te).float().double(), T(Rg).float().double(), T(tg).float().double())
    assert f_d.dtype == torch.float32 and torch.equal(f_t.reshape(-1), w_t.cpu()) and torch.equal(f_d, w_d.cpu().float())


def test_device_median_is_numpys():
    rng = np.random.default_rng(3)
    for n, keep in ((0, 0), (1, 0), (1, 1), (2, 2), (7, 4), (7, 5), (8, 8)):
        v = rng.standard_normal(n)
        k = np.zeros(n, bool)
        k[rng.permutation(n)[:keep]] = True
        v[~k] = np.nan
        for dt in (np.float32, np.float64):
            got = L._median(torch.from_numpy(v.astype(dt)).cuda(), torch.from_numpy(k).cuda()).cpu().numpy()
            want = np.median(v.astype(dt)[k]) if keep else dt("nan")
            assert got.dtype == dt and (got == want or (np.isnan(got) and np.isnan(want))), (n, keep, got, want)


# ---- the batched driver ---------------------------------------------------------------------------------------------------
CAMERA = {"model": "PINHOLE", "width": 64, "height": 48, "params": [40.0, 40.0, 31.5, 23.5]}


@pytest.fixture(scope="module")
def scene():
    """a 6 x 5 x 3 m room of 2000 key Gaussians seen by a 64 x 48 camera (tests/golden/make_golden_matching.py), four database
    frames (the third sees nothing) and a FeatureDecoder with seeded weights"""
    from splatloc_amd.decoder import FeatureDecoder
    from tests import decoder_reference as DR
    from tests.golden.make_golden_matching import FH, FK, FW, look_at, ray_depth, wall_points
    rng = np.random.default_rng(77)
    pts = wall_points(rng, 2000).astype(np.float32)
    marker = rng.uniform(0.004, 0.02, size=(len(pts), 1)).astype(np.float32)
    poses = [look_at(np.array([1.5, 1.2, 1.4]), np.array([5.5, 4.0, 1.2])),
             look_at(np.array([4.5, 3.8, 1.6]), np.array([0.5, 0.8, 1.0])),
             look_at(np.array([-5.0, -5.0, 1.0]), np.array([-10.0, -10.0, 1.0])),     # outside, looking away: no candidates
             look_at(np.array([3.0, 1.0, 1.2]), np.array([3.2, 4.9, 1.8]))]
    frames = []
    for i, c2w in enumerate(poses):
        c2w = c2w.astype(np.float32)
        depth = np.ones((FH, FW), np.float32) if i == 2 else ray_depth(c2w.astype(np.float64), FK, FW, FH).astype(np.float32)
        frames.append({"K": FK, "c2w": torch.from_numpy(c2w), "w2c": torch.from_numpy(np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)),
                       "depth": torch.from_numpy(depth), "sp_kp_mask": torch.from_numpy((rng.random((FH, FW)) < 0.3).astype(np.int32))})
    cfg = DR.office_0_config()
    cfg["scene"] = {"bound": [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]], "voxel_sdf": 0.06}
    torch.manual_seed(0)
    decoder = DR.trained_scale_(FeatureDecoder(cfg).cuda())
    subset = pts[np.sort(rng.choice(len(pts), 1200, replace=False))].astype(np.float64)
    return {"pts": pts, "marker": marker, "frames": frames, "poses": poses, "decoder": decoder, "subset": subset, "K": FK, "W": FW,
            "H": FH}


def _queries(sc, subset, seed):
    """seven queries: 0 and 1 share frame 0, 2 retrieves the frame without candidates, 3 has no keypoints, 4 has three, 5 and 6
    have frames 1 and 3 to themselves.  Keypoints are projections of candidate points under a planted pose near the frame's,
    descriptors the decoder's rows plus noise."""
    rng = np.random.default_rng(seed)
    db_index = [0, 0, 2, 1, 1, 1, 3]
    K, W, H = sc["K"], sc["W"], sc["H"]
    cache, queries, gt = {}, [], []
    for qi, f in enumerate(db_index):
        if f not in cache:
            with torch.no_grad():
                cache[f] = M.get_frusm_pts(sc["pts"], sc["marker"], sc["frames"][f], K, W, H, sc["decoder"], subset=subset)
        p3, f3, _ = cache[f]
        c2w = sc["poses"][f].copy()
        c2w[:3, 3] += rng.uniform(-0.08, 0.08, size=3)
        a = rng.uniform(-0.04, 0.04)
        c2w[:3, :3] = c2w[:3, :3] @ np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        gt.append(c2w)
        if len(p3) < 5 or qi == 3:
            n = 0 if qi == 3 else 12
            queries.append({"keypoints": rng.uniform(0, [W, H], size=(n, 2)).astype(np.float32),
                            "descriptors": rng.standard_normal((256, n)).astype(np.float32)})
            continue
        _, first = np.unique(np.asarray(p3, np.float64), axis=0, return_index=True)
        w2c = np.linalg.inv(c2w)
        pc = np.asarray(p3, np.float64)[first] @ w2c[:3, :3].T + w2c[:3, 3]
        uv = pc[:, :2] / pc[:, 2:] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
        vis = first[(pc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)]
        uv = uv[(pc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)]
        n = 3 if qi == 4 else min(len(vis), 40 + 7 * qi)
        pick = rng.permutation(len(vis))[:n]
        kp = (uv[pick] + rng.normal(size=(n, 2)) * 0.05).astype(np.float32)
        desc = f3.cpu().numpy()[vis[pick]] + 0.02 * rng.standard_normal((n, 256)).astype(np.float32)
        if qi not in (3, 4):   # distractors
            kp = np.concatenate([kp, rng.uniform(0, [W, H], size=(6, 2)).astype(np.float32)])
            desc = np.concatenate([desc, rng.standard_normal((6, 256)).astype(np.float32)])
        queries.append({"keypoints": kp, "descriptors": np.ascontiguousarray(desc.T)})
    return queries, db_index, np.stack(gt), cache


def _per_query(sc, subset, q, cand):
    """INTEGRATION.md §17 and §18, as test.py's match_feature strings them together"""
    p3, f3, _ = cand
    if p3.shape[0] < 5:
        return None
    out = M.HungarianMatcher()({"query_descs": torch.from_numpy(q["descriptors"]), "train_descs": f3.T})
    m = out["matches"].numpy()
    mq, m3 = q["keypoints"][m[0]], p3[m[1]]
    keep = m3[:, 2] > -10000
    return P.solve_pose(mq[keep], m3[keep], CAMERA)


@pytest.mark.parametrize("mode", ("key", "subset"))
def test_localize_is_the_per_query_path_bit_for_bit(scene, mode):
    sc = scene
    subset = sc["subset"] if mode == "subset" else None
    queries, db_index, gt, cand = _queries(sc, subset, 5 if mode == "key" else 6)
    loc = L.Localizer(sc["pts"], sc["marker"], sc["decoder"], sc["K"], sc["W"], sc["H"], CAMERA, subset=subset)
    res = loc.localize(queries, sc["frames"], db_index)
    assert all(res[k].is_cuda for k in res) and res["R_c2w"].dtype == res["t_c2w"].dtype == torch.float64
    assert tuple(res["R_c2w"].shape) == (7, 3, 3) and tuple(res["t_c2w"].shape) == (7, 3)
    assert res["success"].dtype == torch.bool and res["num_inliers"].dtype == torch.int32
    want_ok = [True, True, False, False, False, True, True]
    assert res["success"].cpu().tolist() == want_ok
    for qi, q in enumerate(queries):
        single = _per_query(sc, subset, q, cand[db_index[qi]])
        c2w = sc["frames"][db_index[qi]]["c2w"].double()
        assert torch.equal(res["retrieval_R"][qi].cpu(), c2w[:3, :3]) and torch.equal(res["retrieval_t"][qi].cpu(), c2w[:3, 3])
        if not want_ok[qi]:
            assert single is None or not single[2]["success"]
            assert int(res["num_inliers"][qi]) == 0
            assert torch.equal(res["R_c2w"][qi].cpu(), c2w[:3, :3]) and torch.equal(res["t_c2w"][qi].cpu(), c2w[:3, 3])
            continue
        r, t, ret = single
        assert ret["success"]
        assert torch.equal(res["R_c2w"][qi].cpu(), torch.from_numpy(r)), qi
        assert torch.equal(res["t_c2w"][qi].cpu(), torch.from_numpy(t)), qi
        assert int(res["num_inliers"][qi]) == ret["num_inliers"]
    # the degenerate queries do not change their neighbours: the good ones alone give the same bits
    good = [0, 1, 5, 6]
    alone = loc.localize([queries[i] for i in good], sc["frames"], [db_index[i] for i in good])
    for k in ("R_c2w", "t_c2w", "success", "num_inliers"):
        assert torch.equal(alone[k], res[k][good]), k
    # chunked cost matrices (one LSAP launch per query) change nothing either
    small = L.Localizer(sc["pts"], sc["marker"], sc["decoder"], sc["K"], sc["W"], sc["H"], CAMERA, subset=subset, max_cost_elements=1)
    chunked = small.localize(queries, sc["frames"], db_index)
    for k in res:
        assert torch.equal(chunked[k], res[k]), k
    empty = loc.localize([], sc["frames"], [])
    assert tuple(empty["R_c2w"].shape) == (0, 3, 3) and tuple(empty["success"].shape) == (0,)

    # evaluate: the restatement on the same poses, numpy's medians over the successful queries
    rep = loc.evaluate(res, gt)
    ok = np.array(want_ok)
    assert np.array_equal(rep.success, ok)
    cpu = {k: v.cpu().numpy() for k, v in res.items()}
    for name, R, t in (("retrieval", cpu["retrieval_R"], cpu["retrieval_t"]), ("match", cpu["R_c2w"], cpu["t_c2w"])):
        th, ds = LR.pose_errors(R, t, gt[:, :3, :3], gt[:, :3, 3], valid=ok)
        got_t, got_d = getattr(rep, name + "_theta"), getattr(rep, name + "_dist")
        assert got_t.dtype == np.float32 and got_d.dtype == np.float64
        assert np.isnan(got_t[~ok]).all() and np.isnan(got_d[~ok]).all()
        assert np.all(np.abs(got_t[ok].astype(np.float64) - th[ok]) <= LR.theta_bound(th[ok].astype(np.float64)))
        assert np.all(np.abs(got_d[ok] - ds[ok]) <= 4 * np.spacing(ds[ok]))
        mt, md = getattr(rep, f"median_{name}_theta"), getattr(rep, f"median_{name}_dist")
        assert type(mt) is np.float32 and type(md) is np.float64
        assert mt == np.median(got_t[ok]) and md == np.median(got_d[ok])                  # numpy's median of its own values
        assert abs(float(mt) - float(np.median(th[ok]))) <= float(LR.theta_bound(np.median(th[ok]).astype(np.float64)))
        assert abs(md - np.median(ds[ok])) <= 4 * np.spacing(np.median(ds[ok]))
    # the planted poses are recovered better than the retrieval pose
    assert rep.median_match_dist < rep.median_retrieval_dist
    assert rep.format_report() == ("Median Error: \n"
                                   + "Retrieval: Trans.(cm): {}. Rotation(deg): {}.\n".format(
                                       np.median(rep.retrieval_dist[ok]) * 100, np.median(rep.retrieval_theta[ok]))
                                   + "Match    : Trans.(cm): {}. Rotation(deg): {}.\n".format(
                                       np.median(rep.match_dist[ok]) * 100, np.median(rep.match_theta[ok])))
