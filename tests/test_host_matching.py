"""2D-3D matching (test.py:247-378) on the host: a numpy restatement of scipy's linear_sum_assignment in the order the device
solver walks it, checked against scipy on tie-heavy matrices and against tests/golden/matching.npz
(make_golden_matching.py); the argument errors of splatloc_amd.matching, raised before any device work; and the compiler's
resource report of csrc/matching.hip.  The restatement is also the CPU side of tests/test_gpu_matching.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from splatloc_amd import build as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matching.npz")


def golden():
    return dict(np.load(GOLDEN))


def lsap_restated(cost, maximize=False, return_steps=False):
    """scipy's linear_sum_assignment (Crouse's LAPJV), step for step as csrc/matching.hip runs it"""
    c = np.asarray(cost, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError(f"expected a matrix (2-D array), got a {c.ndim} array")
    tr = c.shape[1] < c.shape[0]
    if tr:
        c = c.T
    if maximize:
        c = -c
    if np.isnan(c).any() or (c == -np.inf).any():
        raise ValueError("matrix contains invalid numeric entries")
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    r4c, c4r, path = np.full(nc, -1), np.full(nr, -1), np.full(nc, -1)
    steps = 0
    for cur in range(nr):
        rem = np.arange(nc - 1, -1, -1)
        num = nc
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        spc = np.full(nc, np.inf)
        minVal, i, sink = 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            js = rem[:num]
            r = ((minVal + c[i, js]) - u[i]) - v[js]
            better = r < spc[js]
            path[js[better]] = i
            spc[js] = np.where(better, r, spc[js])
            s = spc[js]
            lowest = s.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            cand = np.flatnonzero(s == lowest)
            free = cand[r4c[js[cand]] == -1]
            index = free.max() if len(free) else cand.min()
            steps += 1
            minVal = lowest
            j = rem[index]
            if r4c[j] == -1:
                sink = j
            else:
                i = r4c[j]
            SC[j] = True
            num -= 1
            rem[index] = rem[num]
        u[cur] += minVal
        for ii in np.flatnonzero(SR):
            if ii != cur:
                u[ii] += minVal - spc[c4r[ii]]
        for jj in np.flatnonzero(SC):
            v[jj] -= minVal - spc[jj]
        j = sink
        while True:
            ii = path[j]
            r4c[j] = ii
            j, c4r[ii] = c4r[ii], j
            if ii == cur:
                break
    if tr:
        order = np.argsort(c4r)
        out = (c4r[order], order)
    else:
        out = (np.arange(nr), c4r)
    return (out[0], out[1], steps) if return_steps else out


def random_tie_heavy(rng, k):
    shape = (int(rng.integers(1, 13)), int(rng.integers(1, 13)))
    kind = k % 5
    if kind == 0:
        c = rng.integers(0, 3, size=shape).astype(np.float64)
    elif kind == 1:
        c = np.where(rng.random(shape) < 0.5, 1.0, 0.0)
    elif kind == 2:
        s = rng.random(shape).astype(np.float32)
        s[s < 0.4] = 0
        c = (1 - s).astype(np.float64)
    elif kind == 3:
        c = np.full(shape, 1.0)
    else:
        c = rng.integers(-2, 3, size=shape).astype(np.float64)
        c[rng.random(shape) < (0.25 if k % 2 else 0.75)] = np.inf
    return c


def test_restatement_equals_scipy_on_tie_heavy_matrices():
    scipy_opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    infeasible = 0
    for k in range(480):
        c = random_tie_heavy(rng, k)
        mx = bool(k % 3 == 1) and not np.isinf(c).any()
        try:
            want = scipy_opt.linear_sum_assignment(c, maximize=mx)
        except ValueError as e:
            with pytest.raises(ValueError, match=str(e)):
                lsap_restated(c, mx)
            infeasible += 1
            continue
        got = lsap_restated(c, mx)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, c, mx)
    assert infeasible > 0   # both sides of +inf are covered


def test_restatement_rejects_like_scipy():
    for bad in (np.array([[0.0, np.nan]]), np.array([[-np.inf, 1.0]])):
        with pytest.raises(ValueError, match="invalid numeric entries"):
            lsap_restated(bad)
    with pytest.raises(ValueError, match="invalid numeric entries"):
        lsap_restated(np.array([[np.inf, 1.0]]), maximize=True)
    with pytest.raises(ValueError, match="infeasible"):
        lsap_restated(np.array([[np.inf, np.inf], [1.0, 2.0]]))


def test_restatement_reproduces_fixture_solver_cases():
    g = golden()
    for k in range(int(g["l_count"])):
        r, c = lsap_restated(g[f"l{k}_cost"], bool(g[f"l{k}_max"]))
        assert np.array_equal(r, g[f"l{k}_rows"]) and np.array_equal(c, g[f"l{k}_cols"]), k


def reference_cost(d1, d2):
    """hungarian_solve's cost in f64 from f32 similarities computed in f64 and rounded (the fixture's seeds are immune)"""
    a = d1.astype(np.float64) / np.maximum(np.linalg.norm(d1.astype(np.float64), axis=0), 1e-12)
    b = d2.astype(np.float64) / np.maximum(np.linalg.norm(d2.astype(np.float64), axis=0), 1e-12)
    s = (a.T @ b).astype(np.float32)
    s[s < np.float32(0.4)] = 0
    return (np.float32(1) - s).astype(np.float64), s


def test_restatement_reproduces_fixture_hungarian_cases():
    g = golden()
    for k in range(int(g["h_count"])):
        cost, s = reference_cost(g[f"h{k}_d1"], g[f"h{k}_d2"])
        r, c = lsap_restated(cost)
        assert np.array_equal(np.stack([r, c]), g[f"h{k}_matches"]), k
        assert np.abs(s[r, c] - g[f"h{k}_sims"]).max() <= 1e-6


def test_constant_matrix_gives_identity():
    for shape in ((5, 5), (3, 8), (8, 3)):
        r, c = lsap_restated(np.ones(shape))
        n = min(shape)
        assert np.array_equal(r, np.arange(n)) and np.array_equal(c, np.arange(n))


def test_argument_errors_before_device_work():
    from splatloc_amd import matching as M
    with pytest.raises(ValueError, match="2-D"):
        M.linear_sum_assignment(np.zeros(3))
    with pytest.raises(ValueError, match="float32 or float64"):
        M.linear_sum_assignment(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="65535"):
        M.linear_sum_assignment(np.zeros((1, 70000)))
    with pytest.raises(ValueError, match="2\\^31"):
        M.linear_sum_assignment_batch([np.zeros((1, 2)), np.broadcast_to(np.zeros(1), (40000, 60000))])
    with pytest.raises(ValueError, match="dimensions differ"):
        M.match_descriptors(np.zeros((8, 3), np.float32), np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="dimensions differ"):
        M.hungarian_solve(np.zeros((8, 3), np.float32), np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="float32 or float64"):
        M.match_descriptors(np.zeros((8, 3), np.int32), np.zeros((8, 3), np.int32))
    with pytest.raises(ValueError, match="not exist"):
        M.HungarianMatcher()({"query_descs": np.zeros((8, 3), np.float32)})
    with pytest.raises(ValueError, match="points must be"):
        M.frustum_candidates(np.zeros((5, 2), np.float32), np.eye(4), np.eye(3), 64, 48)
    with pytest.raises(ValueError, match="w2c"):
        M.frustum_candidates(np.zeros((5, 3), np.float32), np.eye(3), np.eye(3), 64, 48)
    with pytest.raises(ValueError, match="needs kp_mask"):
        M.frustum_candidates(np.zeros((5, 3), np.float32), np.eye(4), np.eye(3), 64, 48, marker=np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="marker must hold"):
        M.frustum_candidates(np.zeros((5, 3), np.float32), np.eye(4), np.eye(3), 64, 48, marker=np.zeros(4, np.float32))


def test_frustum_restatement_reproduces_fixture():
    from tests import matching_reference as R
    g = golden()
    W, H = (int(x) for x in g["f_size"])
    idx, xyz, uv = R.frustum_restated(g["f_points"], g["f_w2c"], g["f_K"], W, H, marker=g["f_marker"], kp_mask=g["f_mask"],
                                      depth=g["f_depth"], c2w=g["f_c2w"], kp_K=g["f_K"])
    assert len(idx) == 600 and np.array_equal(idx, g["f_idx"])
    assert xyz.dtype == np.float32 and np.array_equal(xyz, g["f_pts3d"])
    assert np.abs(uv - g["f_pts2d"]).max() <= 1e-4   # the reference's key mode projects in f32
    idx, xyz, uv = R.frustum_restated(g["s_subset"], g["f_w2c"], g["f_K"], W, H)
    assert len(idx) == 1074 and np.array_equal(idx, g["s_idx"])
    assert np.array_equal(xyz.astype(np.float64), g["s_pts3d"])
    assert np.abs(uv - g["s_pts2d"]).max() <= 1e-12


def test_frustum_restatement_equals_kdtree_away_from_the_edges():
    """scipy's k-d tree (the reference's search) on duplicate-free scenes: equal pairs wherever the nearest distance is not
    within 1e-9 of the 0.1 m bound and the runner-up is not within 1e-9 of the nearest"""
    spatial = pytest.importorskip("scipy.spatial")
    from tests import matching_reference as R
    pairs = 0
    for seed, N, W, H, density in ((1, 2049, 64, 48, 0.3), (2, 1025, 17, 9, 1.0), (3, 300, 250, 130, 0.3)):
        s = R.room_scene(seed, N, W, H, density)
        assert len(np.unique(s["points"], axis=0)) == N
        idx, _, _, dist = R.frustum_restated(s["points"], s["w2c"], s["K"], W, H, return_distance=True, **R.key_args(s))
        pz, u, v = R.project(s["points"], s["w2c"], s["K"])
        kept = np.flatnonzero((pz > 0.05) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (s["marker"] > np.float32(0.005)))
        q, ok = R.backproject(s["mask"], s["depth"], s["c2w"], s["K"])
        assert ok.all()
        d2, i2 = spatial.cKDTree(s["points"][kept].astype(np.float64)).query(q, k=2)
        safe = (np.abs(d2[:, 0] - 0.1) > 1e-9) & (d2[:, 1] - d2[:, 0] > 1e-9)
        assert safe.mean() > 0.99
        dk, ik = spatial.cKDTree(s["points"][kept].astype(np.float64)).query(q, distance_upper_bound=0.1)
        found = np.isfinite(dk)
        want = np.where(found, kept[np.minimum(ik, len(kept) - 1)], -1)
        # the restatement's pairs, one slot per keypoint
        d1, p1 = R.nearest(s["points"][kept].astype(np.float64), q)
        got = np.where(d1 < 0.1, kept[p1], -1)
        assert np.array_equal(got[safe], want[safe]), seed
        assert np.array_equal(idx, got[got >= 0]) and np.array_equal(dist, d1[got >= 0])
        assert 0 < (got >= 0).sum() < len(q)   # both outcomes of d < 0.1
        pairs += int((got >= 0).sum())
    assert pairs > 500


def test_cost_f64_reproduces_fixture_hungarian_cases():
    from tests import matching_reference as R
    g = golden()
    for k in range(int(g["h_count"])):
        d1, d2 = g[f"h{k}_d1"], g[f"h{k}_d2"]
        want, s = reference_cost(d1, d2)
        sim, cost = R.cost_f64(d1, d2, 0.4)
        if d2.shape[1] < d1.shape[1]:
            sim, cost = sim.T, cost.T
        assert sim.shape == want.shape
        s32 = sim.astype(np.float32)
        s32[s32 < np.float32(0.4)] = 0
        assert np.array_equal(s32, s) and np.array_equal((np.float32(1) - s32).astype(np.float64), want), k
        assert np.abs(cost - want).max() <= 2.0 ** -24   # the f32 rounding of sim and of 1 - sim below 1
        r, c = lsap_restated(cost)
        assert np.array_equal(np.stack([r, c]), g[f"h{k}_matches"]), k


def test_cost_cases_leave_the_threshold_band_nearly_empty():
    """the differential cost test of tests/test_gpu_matching_edges.py may skip at most 0.1 % of a case's entries"""
    from tests import matching_reference as R
    assert R.cost_bound(256) == 520 * 2.0 ** -24
    for D, N1, N2 in R.cost_cases():
        d1, d2 = R.cost_case(D, N1, N2)
        sim, cost = R.cost_f64(d1, d2, R.COST_THRESHOLD)
        assert sim.shape == (min(N1, N2), max(N1, N2))
        assert R.band(sim, R.COST_THRESHOLD, D).mean() <= R.BAND_SHARE, (D, N1, N2)
        # numpy's own f32 evaluation stays inside the derived bound
        a = (d1 / np.maximum(np.linalg.norm(d1, axis=0), np.float32(1e-12))).astype(np.float32)
        b = (d2 / np.maximum(np.linalg.norm(d2, axis=0), np.float32(1e-12))).astype(np.float32)
        s32 = (a.T @ b).astype(np.float64)
        assert np.abs((s32.T if N2 < N1 else s32) - sim).max() <= R.cost_bound(D), (D, N1, N2)


def _usage(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = [*B.COMMON, "-ffp-contract=off"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    return usage


def test_matching_kernels_have_no_scratch_and_no_spills():
    usage = _usage("matching.hip")
    assert len(usage) >= 11, sorted(usage)
    assert any("lsap_kernel" in k for k in usage)
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 160 * 1024, (name, u)
