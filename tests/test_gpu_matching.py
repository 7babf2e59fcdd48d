"""2D-3D matching on the MI355X (csrc/matching.hip through splatloc_amd.matching) against the reference's own numbers
(tests/golden/matching.npz), scipy's indices and the restatement of tests/test_host_matching.py."""
import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import matching as M
from tests.golden.make_golden_matching import big_cost
from tests.test_host_matching import golden, lsap_restated

pytestmark = pytest.mark.gpu


def _np(pair):
    return tuple(x.cpu().numpy() for x in pair)


def _same(got, rows, cols):
    r, c = _np(got)
    return np.array_equal(r, rows) and np.array_equal(c, cols)


@pytest.fixture
def global_path():
    lib = _native.load()
    lib.splatraster_debug_set_lsap_lds(0)
    yield
    lib.splatraster_debug_set_lsap_lds(1)


def test_solver_matches_fixture_indices_f64_and_f32():
    g = golden()
    for k in range(int(g["l_count"])):
        c, mx = g[f"l{k}_cost"], bool(g[f"l{k}_max"])
        assert _same(M.linear_sum_assignment(c, maximize=mx), g[f"l{k}_rows"], g[f"l{k}_cols"]), k
        # f32 input: the fixture's costs are exact in f32 (quarters, f32 similarities, +inf)
        if np.array_equal(c.astype(np.float32).astype(np.float64), c):
            got = M.linear_sum_assignment(torch.from_numpy(c.astype(np.float32)).cuda(), maximize=mx)
            assert _same(got, g[f"l{k}_rows"], g[f"l{k}_cols"]), k


def test_solver_shapes_and_constant_identity():
    for shape in ((1, 1), (1, 9), (9, 1), (6, 6), (4, 10), (10, 4)):
        r, c = _np(M.linear_sum_assignment(np.ones(shape)))
        n = min(shape)
        assert np.array_equal(r, np.arange(n)) and np.array_equal(c, np.arange(n)), shape   # scipy #11602
    r, c = _np(M.linear_sum_assignment(np.zeros((0, 5))))
    assert r.shape == c.shape == (0,)


def test_lds_and_global_paths_agree(global_path):
    rng = np.random.default_rng(3)
    cases = []
    for shape in ((40, 900), (700, 1024), (300, 1100), (1200, 4096), (50, 4200), (4200, 30)):
        s = rng.random(shape) ** 2
        cases.append(1.0 - np.where(s < 0.4, 0.0, s))
    lib = _native.load()
    forced = [_np(M.linear_sum_assignment(c)) for c in cases]
    lib.splatraster_debug_set_lsap_lds(1)
    auto = [_np(M.linear_sum_assignment(c)) for c in cases]
    for c, (fr, fc), (ar, ac) in zip(cases, forced, auto):
        assert np.array_equal(fr, ar) and np.array_equal(fc, ac), c.shape
    for c, (ar, ac) in zip(cases[:3], auto[:3]):
        r, cc = lsap_restated(c)
        assert np.array_equal(ar, r) and np.array_equal(ac, cc), c.shape


def test_batch_equals_single_calls():
    rng = np.random.default_rng(4)
    mats = []
    for k in range(70):   # more than one launch chunk, mixed LDS variants and orientations
        shape = (int(rng.integers(1, 60)), int(rng.integers(1, 60))) if k % 9 else (int(rng.integers(100, 300)), 1500)
        mats.append(np.where(rng.random(shape) < 0.6, 1.0, rng.integers(0, 5, size=shape) / 4.0))
    out, steps = M.linear_sum_assignment_batch(mats, return_steps=True)
    assert len(out) == len(mats) == len(steps)
    for c, (r, cc), s in zip(mats, out, steps):
        r1, c1, s1 = M.linear_sum_assignment(c, return_steps=True)
        assert np.array_equal(r.cpu().numpy(), r1.cpu().numpy()) and np.array_equal(cc.cpu().numpy(), c1.cpu().numpy())
        assert s == s1
    for c, (r, cc) in list(zip(mats, out))[:20]:
        rr, rc = lsap_restated(c)
        assert np.array_equal(r.cpu().numpy(), rr) and np.array_equal(cc.cpu().numpy(), rc)


def test_big_seed_case():
    g = golden()
    c = big_cost(int(g["big_seed"]), tuple(int(x) for x in g["big_shape"]))
    assert _same(M.linear_sum_assignment(c), g["big_rows"], g["big_cols"])


def test_solver_errors():
    for bad in (np.array([[0.0, np.nan], [1.0, 2.0]]), np.array([[-np.inf, 1.0]])):
        with pytest.raises(ValueError, match="invalid numeric entries"):
            M.linear_sum_assignment(bad)
    with pytest.raises(ValueError, match="invalid numeric entries"):
        M.linear_sum_assignment(np.array([[np.inf, 1.0]]), maximize=True)
    with pytest.raises(ValueError, match="infeasible"):
        M.linear_sum_assignment(np.array([[np.inf, np.inf], [1.0, 2.0]]))
    # scipy checks the entries first: an invalid entry after an infeasible row is still "invalid"
    with pytest.raises(ValueError, match="invalid numeric entries"):
        M.linear_sum_assignment(np.array([[np.inf, np.inf], [1.0, np.nan]]))


def test_hungarian_drop_in_matches_reference_fixture():
    g = golden()
    for k in range(int(g["h_count"])):
        d1, d2 = torch.from_numpy(g[f"h{k}_d1"]), torch.from_numpy(g[f"h{k}_d2"])
        m, s = M.hungarian_solve(d1, d2)
        assert m.device.type == "cpu" and m.dtype == torch.int64 and s.dtype == torch.float32
        assert np.array_equal(m.numpy(), g[f"h{k}_matches"]), k
        assert np.abs(s.numpy() - g[f"h{k}_sims"]).max() <= 1e-6, k
        out = M.HungarianMatcher()({"query_descs": d1, "train_descs": d2.cuda()})
        assert np.array_equal(out["matches"].numpy(), g[f"h{k}_matches"])


def test_device_assignment_is_optimal_on_its_own_cost():
    rng = np.random.default_rng(9)
    for D, N1, N2 in ((256, 300, 200), (256, 200, 450), (64, 400, 400)):
        d1 = torch.from_numpy(rng.standard_normal((D, N1)).astype(np.float32)).cuda()
        d2 = torch.from_numpy(rng.standard_normal((D, N2)).astype(np.float32)).cuda()
        d2[:, : min(N1, N2) // 2] += d1[:, : min(N1, N2) // 2] * 2
        m, s = M.match_descriptors(d1, d2)
        # the device's own cost matrix, from its own similarities of every pair
        lib = _native.load()
        a, b = d1.contiguous(), d2.contiguous()
        norms = torch.empty(N1 + N2, dtype=torch.float32, device="cuda")
        cost = torch.empty(N1 * N2, dtype=torch.float64, device="cuda")
        from splatloc_amd.rasterizer import _stream
        st = lib.splatraster_match_cost(D, N1, N2, M._ptr(a), M._ptr(b), 0.4, M._ptr(norms), M._ptr(cost),
                                        _stream(torch.device("cuda", 0)))
        assert st == 0
        cm = cost.cpu().numpy().reshape((N1, N2) if N1 <= N2 else (N2, N1))
        cm = cm if N1 <= N2 else cm.T
        r, c = lsap_restated(cm)
        mm = m.cpu().numpy()
        assert cm[mm[0], mm[1]].sum() == cm[r, c].sum()
        assert np.array_equal(mm, np.stack([r, c]))
        # sims are the matrix's own entries
        assert np.array_equal((1.0 - s.cpu().numpy().astype(np.float32)).astype(np.float32),
                              cm[mm[0], mm[1]].astype(np.float32))


def test_empty_descriptors_give_empty_matches():
    m, s = M.hungarian_solve(torch.zeros(8, 0), torch.zeros(8, 5))
    assert tuple(m.shape) == (2, 0) and tuple(s.shape) == (0,)


def _frame(g):
    return {"w2c": torch.from_numpy(g["f_w2c"]), "c2w": torch.from_numpy(g["f_c2w"]), "K": g["f_K"],
            "depth": torch.from_numpy(g["f_depth"]), "sp_kp_mask": torch.from_numpy(g["f_mask"])}


def test_frustum_key_mode_matches_fixture():
    g = golden()
    W, H = (int(x) for x in g["f_size"])
    idx, xyz, uv = M.frustum_candidates(g["f_points"], g["f_w2c"], g["f_K"], W, H, marker=g["f_marker"],
                                        kp_mask=g["f_mask"], depth=g["f_depth"], c2w=g["f_c2w"], kp_K=g["f_K"])
    assert np.array_equal(idx.cpu().numpy(), g["f_idx"])
    assert np.array_equal(xyz.cpu().numpy(), g["f_pts3d"])
    assert np.abs(uv.cpu().numpy() - g["f_pts2d"]).max() <= 1e-4
    p3, f3, p2 = M.get_frusm_pts(torch.from_numpy(g["f_points"]).cuda(), torch.from_numpy(g["f_marker"]), _frame(g),
                                 g["f_K"], W, H, decoder=lambda x: x)
    assert p3.dtype == np.float32 and p2.dtype == np.float64
    assert np.array_equal(p3, g["f_pts3d"]) and np.array_equal(f3.numpy(), g["f_pts3d"])
    assert np.abs(p2 - g["f_pts2d"]).max() <= 1e-4


def test_frustum_subset_mode_matches_fixture():
    g = golden()
    W, H = (int(x) for x in g["f_size"])
    idx, xyz, uv = M.frustum_candidates(g["s_subset"], g["f_w2c"], g["f_K"], W, H)
    assert np.array_equal(idx.cpu().numpy(), g["s_idx"])
    assert np.array_equal(xyz.cpu().numpy().astype(np.float64), g["s_pts3d"])
    assert np.abs(uv.cpu().numpy() - g["s_pts2d"]).max() <= 1e-4
    p3, _, p2 = M.get_frusm_pts(None, None, _frame(g), g["f_K"], W, H, decoder=lambda x: x, subset=g["s_subset"])
    assert p3.dtype == np.float64 and np.array_equal(p3, g["s_pts3d"])


def test_everything_runs_on_a_side_stream():
    g = golden()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = M.linear_sum_assignment(g["l10_cost"], maximize=bool(g["l10_max"]))
        m, _ = M.hungarian_solve(torch.from_numpy(g["h0_d1"]).cuda(), torch.from_numpy(g["h0_d2"]).cuda())
        W, H = (int(x) for x in g["f_size"])
        idx, _, _ = M.frustum_candidates(g["s_subset"], g["f_w2c"], g["f_K"], W, H)
    s.synchronize()
    assert _same(out, g["l10_rows"], g["l10_cols"])
    assert np.array_equal(m.numpy(), g["h0_matches"])
    assert np.array_equal(idx.cpu().numpy(), g["s_idx"])
