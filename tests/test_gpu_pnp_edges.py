"""csrc/pnp.hip on the MI355X against the f64 restatement of tests/test_host_pnp.py, on the cases of tests/pnp_cases.py: the
whole estimator (best-of-batch, local optimisation, stopping rule, inlier mask, Cauchy-loss refinement) rather than the planted
pose, the stopping rule of problems that finish in different batches of one call, more problems than one block of the state
kernel, the rule between models of equal count, the degenerate outcomes, scoring with residuals exactly on the threshold and
z exactly 0, the sampler and P3P at n = 4, 5, trial 2^40 and a negative focal length, and the input layouts.
tests/test_host_pnp.py checks on the CPU that the
restatement's decisions on these cases do not depend on the order of its sums (pose spread 2.4e-15) and that no residual of its
RANSAC model lies within 1e-6 of the threshold, so a device that follows include/splatraster.h differs from it by rounding
only: decisions are compared exactly, poses at 1e-9.

Largest deviation of the device pose from the restatement's over the 17 cases, measured on the MI355X: R 1.0e-15, t 2.6e-15
relative to max(1, |t|), both at n4; the restatement's own spread under reversed sums is 2.4e-15.  Every decision (success,
trials, num_inliers, inlier mask) was equal on every case: the pose stage matched the restatement.
"""
import ctypes as C
import fractions
import itertools

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import pnp as P
from splatloc_amd.rasterizer import _stream
from tests import pnp_cases as cases
from tests import test_host_pnp as H
from tests.test_gpu_pnp import DEV, _bits, _dev, _table, _ws

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_matches_reference(r, ref, what):
    """a device result dict against estimate_restated's: decisions exactly, the refined pose at 1e-9"""
    g = _host(r)
    assert bool(g["success"]) == ref["success"], what
    assert int(g["trials"]) == ref["trials"], (what, int(g["trials"]), ref["trials"])
    assert int(g["num_inliers"]) == ref["num_inliers"], (what, int(g["num_inliers"]), ref["num_inliers"])
    assert g["inliers"].dtype == np.bool_ and np.array_equal(g["inliers"], ref["inliers"]), what
    assert int(g["num_inliers"]) == int(g["inliers"].sum()), what
    dR, dt = cases.pose_deviation(g["R"], g["t"], ref)
    print(f"pnp-deviation {what}: R {dR:.3e} t {dt:.3e}")
    assert dR <= TOL and dt <= TOL, (what, dR, dt)


def _solve_case(name, **override):
    p2d, p3d, _, K = cases.scene(name)
    return P.estimate_absolute_pose(p2d, p3d, K, seed=cases.SEED, **{**cases.BY_NAME[name].options, **override})


# ---- the whole estimator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_estimator_matches_restatement(name):
    case, ref = cases.BY_NAME[name], cases.reference(name)
    assert ref["success"] and ref["trials"] == case.trials
    p2d = cases.scene(name)[0]
    assert p2d.dtype == (np.float32 if case.f32 else np.float64)
    _assert_matches_reference(_solve_case(name), ref, name)


def test_equal_counts_are_decided_by_the_smaller_sum():
    """two poses with 20 inliers each: the pose whose model has the smallest residual sum is returned, not the other one
    (tests/test_host_pnp.py checks that the largest sum of the tied models belongs to the other pose)"""
    p2d, p3d, _, K, _ = cases.tie_scene()
    _assert_matches_reference(P.estimate_absolute_pose(p2d, p3d, K, seed=cases.SEED, **cases.TIE_OPTIONS), cases.tie_reference(),
                              "two poses")


# ---- stopping rule across a batch ---------------------------------------------------------------------------------------
BATCH_NAMES = ("n5", "share80", "share90", "max1500", "ratio", "n1025")
# One call has one set of options, so the six scenes are solved under the options of share90, max1500 and ratio in turn: each
# of the three finishes after its own 5, 2 and 3 batches next to problems that finish earlier.  Batches per problem, from the
# trial rule at the planted inlier shares (1, 0.2, 0.1, 0.5, 0.3, 0.7 of n):
BATCH_OPTIONS = {"share90": (1, 2, 5, 1, 1, 1), "max1500": (2, 2, 2, 2, 2, 2), "ratio": (1, 3, 3, 1, 3, 1)}


@pytest.mark.parametrize("options_of", sorted(BATCH_OPTIONS))
def test_problems_of_one_call_stop_in_different_batches(options_of):
    opts = cases.BY_NAME[options_of].options
    probs, refs = [], []
    for name in BATCH_NAMES:
        p2d, p3d, intr, K = cases.scene(name)
        probs.append((p2d, p3d, K))
        same = cases.BY_NAME[name].options == opts
        refs.append(cases.reference(name) if same else
                    H.estimate_restated(p2d, p3d, intr, seed=cases.SEED, **cases.reference_options(opts)))
    assert tuple(r["trials"] // H.BATCH for r in refs) == BATCH_OPTIONS[options_of]
    batch = P.estimate_absolute_pose_batch(probs, seed=cases.SEED, **opts)
    for name, prob, got, ref in zip(BATCH_NAMES, probs, batch, refs):
        single = P.estimate_absolute_pose(*prob, seed=cases.SEED, **opts)
        assert _bits(got) == _bits(single), name
        _assert_matches_reference(got, ref, f"{name} under the options of {options_of}")


# ---- more problems than one block ---------------------------------------------------------------------------------------
def _small_problem(b):
    n = 4 + b % 5
    p2d, p3d, _, _, _, intr, _ = H.planted_scene(9100 + b, n, 0.0, H.SCENE12 if b % 2 else H.REPLICA, noise=0.5)
    return p2d, p3d, intr


def test_more_problems_than_one_block():
    """260 problems: past one 256-thread block of pnp_init_kernel and one stride of pnp_state_kernel"""
    B = 260
    items = [_small_problem(b) for b in range(B)]
    probs = [(p2d, p3d, cases.intrinsics_matrix(intr)) for p2d, p3d, intr in items]
    out = P.estimate_absolute_pose_batch(probs, seed=cases.SEED)
    assert len(out) == B
    success = torch.stack([r["success"] for r in out]).cpu().numpy()
    trials = torch.stack([r["trials"] for r in out]).cpu().numpy()
    ninl = torch.stack([r["num_inliers"] for r in out]).cpu().numpy()
    mask = torch.cat([r["inliers"] for r in out]).cpu().numpy()
    n = np.array([len(p2d) for p2d, _, _ in items])
    assert success.all(), np.flatnonzero(~success)
    assert np.array_equal(trials, np.full(B, 1024))
    assert np.array_equal(ninl, n), np.flatnonzero(ninl != n)
    assert mask.shape == (n.sum(),) and mask.all()
    for b in (0, 1, 255, 256, 259):
        p2d, p3d, intr = items[b]
        _assert_matches_reference(out[b], H.estimate_restated(p2d, p3d, intr, seed=cases.SEED), f"problem {b} of {B}")
        assert _bits(out[b]) == _bits(P.estimate_absolute_pose(*probs[b], seed=cases.SEED)), b


# ---- degenerate problems ------------------------------------------------------------------------------------------------
def test_degenerate_problems_match_restatement():
    """the collinear and the single-point scene of test_degenerate_inputs_fail_without_nan: no model in 2 batches"""
    rng = np.random.default_rng(8)
    s = rng.uniform(0, 1, size=(200, 1))
    line = np.array([0.0, 0.0, 3.0]) + s * np.array([1.0, 0.5, 0.2])
    uv = rng.uniform(0, 640, size=(200, 2))
    same = np.tile(np.array([[0.3, 0.2, 4.0]]), (100, 1))
    intr = (572.0, 572.0, 320.0, 240.0)
    for p2d, p3d in ((uv, line), (uv[:100], same)):
        ref = H.estimate_restated(p2d, p3d, intr, max_num_trials=2000, seed=cases.SEED)
        assert ref == {"success": False, "trials": 2048}
        g = _host(P.estimate_absolute_pose(p2d, p3d, cases.intrinsics_matrix(intr), max_num_trials=2000, seed=cases.SEED))
        assert not bool(g["success"])
        assert int(g["trials"]) == ref["trials"]
        assert np.isfinite(g["R"]).all() and np.isfinite(g["t"]).all()
        assert g["inliers"].shape == (len(p2d),) and not g["inliers"].any()


# ---- score at exact edges -----------------------------------------------------------------------------------------------
# fx = fy = 128, cx = cy = 8, threshold 12 px.  Under model 0 (R = I, t = 0) X = (0.25, 0, 2) projects to (24, 8) in exact
# arithmetic, so u = 36 gives du = 12 and r = 144 = thr2 exactly.  Point kinds as (X, (u, v)) and their squared residual under
# model 0 and under model 1 (t = (0, 0, -2): z = 0 for every z = 2 point); None: not an inlier.
EDGE_INTR = (128.0, 128.0, 8.0, 8.0)
UP, DOWN = float(np.nextafter(36.0, np.inf)), float(np.nextafter(36.0, -np.inf))
BELOW = fractions.Fraction(144) - fractions.Fraction(6, 2 ** 45)   # fl((12 - 2^-47)^2): 2^-47 is the spacing of f64 at 36
KINDS = {
    "on_u": ((0.25, 0.0, 2.0), (36.0, 8.0), 144, None),        # r == thr2: an inlier
    "on_v": ((0.0, 0.25, 2.0), (8.0, 36.0), 144, None),
    "above_u": ((0.25, 0.0, 2.0), (UP, 8.0), None, None),      # one ulp of u above: not an inlier
    "above_v": ((0.0, 0.25, 2.0), (8.0, UP), None, None),
    "below_u": ((0.25, 0.0, 2.0), (DOWN, 8.0), BELOW, None),   # one ulp below: an inlier
    "below_v": ((0.0, 0.25, 2.0), (8.0, DOWN), BELOW, None),
    "zero": ((0.5, -0.25, 2.0), (40.0, -8.0), 0, None),        # zero residual; model 1: x / 0 = inf
    "centre": ((0.0, 0.0, 2.0), (8.0, 8.0), 0, None),          # model 1: 0 / 0 = NaN
    "behind_u": ((-0.25, 0.0, -2.0), (24.0, 8.0), None, None),  # z < 0 with zero residual: never counts
    "behind_v": ((0.0, -0.25, -2.0), (8.0, 24.0), None, None),
    "one": ((0.25, 0.0, 2.0), (25.0, 8.0), 1, None),
    "four": ((0.25, 0.0, 2.0), (26.0, 8.0), 4, None),
    "nine": ((0.25, 0.0, 2.0), (24.0, 11.0), 9, None),
    "far_on": ((0.25, 0.0, 4.0), (36.0, 8.0), None, 144),      # r == thr2 under model 1, 400 under model 0
    "far_above": ((0.25, 0.0, 4.0), (UP, 8.0), None, None),
    "far_centre": ((0.0, 0.0, 4.0), (8.0, 8.0), 0, 0),
}
# every inlier residual an integer: sums of any order are exact
INTEGER_CYCLE = ("on_u", "on_v", "above_u", "above_v", "zero", "centre", "behind_u", "behind_v", "one", "four", "nine", "far_on",
                 "far_above", "far_centre")
# the one-ulp-below points: their residual is 144 - 3 * 2^-44, so a sum stays exact in any order only below 512; three
# residuals near 144, then kinds that add nothing to the sum of model 0
BELOW_HEAD = ("below_u", "below_v", "on_u", "above_u")
BELOW_CYCLE = ("above_v", "zero", "centre", "behind_u", "behind_v", "far_centre", "far_above", "above_u")
_I = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
EDGE_MODELS = np.array([_I + (0.0, 0.0, 0.0),
                        _I + (0.0, 0.0, -2.0),
                        (-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0),    # half turn about z
                        (1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0),    # half turn about x: z < 0 at z = 2
                        _I + (0.0, 0.0, 2.0)])                                             # z = 0 for the points behind


def _edge_kinds(n, below):
    if not below:
        return [INTEGER_CYCLE[i % len(INTEGER_CYCLE)] for i in range(n)]
    return [BELOW_HEAD[i] if i < len(BELOW_HEAD) else BELOW_CYCLE[(i - len(BELOW_HEAD)) % len(BELOW_CYCLE)] for i in range(n)]


def _edge_points(kinds):
    return np.array([KINDS[k][1] for k in kinds]), np.array([KINDS[k][0] for k in kinds])


def _expected_support(kinds, model):
    """(count, sum) under model 0 or 1 from the table above, in exact arithmetic"""
    rs = [KINDS[k][2 + model] for k in kinds if KINDS[k][2 + model] is not None]
    total = sum(rs, fractions.Fraction(0))
    assert fractions.Fraction(float(total)) == total   # representable
    return len(rs), float(total)


def _device_scores(items, M):
    """count [B, M], sum [B, M] of the first M edge models, the problems packed behind 3 unused points"""
    lib = _native.load()
    pad2, pad3 = np.full((3, 2), 1e6), np.full((3, 3), -1e6)
    probs, off = [], 3
    for p2d, _ in items:
        probs.append(P.PnpProblem(off, len(p2d), 0, *EDGE_INTR))
        off += len(p2d)
    B = len(items)
    tab = (P.PnpProblem * B)(*probs)
    p2 = torch.from_numpy(np.concatenate([pad2] + [a for a, _ in items])).to(DEV)
    p3 = torch.from_numpy(np.concatenate([pad3] + [b for _, b in items])).to(DEV)
    md = torch.from_numpy(np.tile(EDGE_MODELS[:M], (B, 1, 1))).to(DEV)
    opt = P.options(max_error_px=12.0)
    cnt = torch.full((B, M), -7, dtype=torch.int32, device=DEV)
    sm = torch.full((B, M), float("nan"), dtype=torch.float64, device=DEV)
    ws = _ws(lib, B, tab, opt)
    assert lib.splatraster_pnp_score(B, tab, C.byref(opt), M, P._ptr(md), P._ptr(p2), P._ptr(p3), P._ptr(cnt), P._ptr(sm),
                                     P._ptr(ws), _stream(DEV)) == 0
    return cnt.cpu().numpy(), sm.cpu().numpy()


def _assert_edge_scores(problems, M):
    """problems: [(n, below)]; every (b, q) == the table (models 0, 1) and == score of the restatement"""
    kinds = [_edge_kinds(n, below) for n, below in problems]
    items = [_edge_points(k) for k in kinds]
    c, s = _device_scores(items, M)
    assert np.isfinite(s).all()
    for b, ((p2d, p3d), kd) in enumerate(zip(items, kinds)):
        for q in range(M):
            r, z = H.residuals(EDGE_MODELS[q], p2d, p3d, EDGE_INTR)
            rin = r[(z > 0) & (r <= 144.0)]
            # the restatement's own sum is exact: integers, or multiples of 2^-44 that stay below 512
            assert (rin == np.round(rin)).all() or ((rin * 2.0 ** 44 == np.round(rin * 2.0 ** 44)).all() and rin.sum() < 512.0)
            want = H.score(EDGE_MODELS[q], p2d, p3d, EDGE_INTR, 12.0)
            if q < 2:
                assert want == _expected_support(kd, q), (problems[b], q)
            assert (int(c[b, q]), float(s[b, q])) == want, (problems[b], q, c[b, q], s[b, q], want)


@pytest.mark.parametrize("M", (1, 3, 5))
@pytest.mark.parametrize("n", (4, 63, 64, 65, 129))
def test_score_at_exact_edges(n, M):
    for below in (False, True):
        kinds = _edge_kinds(n, below)
        count, total = _expected_support(kinds, 0)
        if below:    # both one-ulp-below points and the point on the threshold count; the sum is no integer
            assert count >= 3 and 431.0 < total < 432.0
        else:        # every point on the threshold counts, none of the points one ulp above
            assert count == sum(KINDS[k][2] is not None for k in kinds) and total == int(total)
            assert total >= 288 and "above_u" in kinds and "above_v" in kinds
        _assert_edge_scores([(n, below)], M)


def test_score_at_exact_edges_in_a_batch():
    _assert_edge_scores([(65, False), (4, True), (129, False)], 5)
    _assert_edge_scores([(129, True), (63, False), (64, False)], 3)


# ---- hypotheses at edges ------------------------------------------------------------------------------------------------
def _hypotheses(items, seed, trial0, T):
    """splatraster_pnp_hypotheses of items [(p2d, p3d, intr)] compared with the restatement as test_hypotheses_match_restatement
    does; returns (samples [B, T, 3], models [B, T, 4, 12], nmodels [B, T])"""
    lib = _native.load()
    B = len(items)
    opt = P.options(seed=seed)
    tab = _table(items)
    p2, p3 = _dev(items)
    samples = torch.full((B, T, 3), -1, dtype=torch.int32, device=DEV)
    models = torch.zeros((B, T, 4, 12), dtype=torch.float64, device=DEV)
    nmod = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    ws = _ws(lib, B, tab, opt)
    assert lib.splatraster_pnp_hypotheses(B, tab, C.byref(opt), trial0, T, P._ptr(p2), P._ptr(p3), P._ptr(samples),
                                          P._ptr(models), P._ptr(nmod), P._ptr(ws), _stream(DEV)) == 0
    s, m, nm = samples.cpu().numpy(), models.cpu().numpy(), nmod.cpu().numpy()
    for b, (a2, a3, intr) in enumerate(items):
        for k in range(T):
            idx, ms = H.hypotheses(a2, a3, intr, seed, trial0 + k)
            assert tuple(s[b, k]) == idx, (b, k)
            assert nm[b, k] == len(ms), (b, k)
            for q, want in enumerate(ms):
                want = np.array(want)
                assert np.isfinite(m[b, k, q]).all()
                assert np.abs(m[b, k, q] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (b, k, q)
    return s, m, nm


def _case_item(name):
    p2d, p3d, intr, _ = cases.scene(name)
    return p2d, p3d, intr


def test_hypotheses_at_the_smallest_n():
    s, _, nm = _hypotheses([_case_item("n4"), _case_item("n5")], 77, 0, 1024)
    for b, n in enumerate((4, 5)):
        assert ((s[b] >= 0) & (s[b] < n)).all()
        assert all(len(set(t)) == 3 for t in s[b].tolist())
    assert {tuple(t) for t in s[0].tolist()} == set(itertools.permutations(range(4), 3))
    assert nm.sum() > 1024


def test_hypotheses_at_trial_2_to_the_40():
    p2d, p3d, _, _, _, intr, _ = H.planted_scene(41, 300, 0.0, H.REPLICA)
    s, _, nm = _hypotheses([(p2d, p3d, intr)], 77, 2 ** 40, 1)
    assert s.shape == (1, 1, 3) and 0 <= nm[0, 0] <= 4


def test_hypotheses_with_a_negative_focal_length():
    camera = {"model": "PINHOLE", "width": 640, "height": 480, "params": [500.0, -430.0, 320.0, 240.0]}
    p2d, p3d, _, _, _, intr, _ = H.planted_scene(42, 50, 0.0, camera)
    assert intr == (500.0, -430.0, 320.0, 240.0)
    _, _, nm = _hypotheses([(p2d, p3d, intr)], 77, 0, 256)
    assert nm.sum() > 256


def test_hypotheses_with_repeated_points():
    """n = 6 with three identical 3D points: a sample with two of them has a zero side and gives no model"""
    p2d, p3d, _, _, _, intr, _ = H.planted_scene(43, 6, 0.0, H.SCENE12)
    p3d = p3d.copy()
    p3d[[1, 3, 4]] = p3d[1]
    s, m, nm = _hypotheses([(p2d, p3d, intr)], 77, 0, 1024)
    twice = np.isin(s[0], (1, 3, 4)).sum(axis=1) >= 2
    assert 100 < twice.sum() < 924
    assert (nm[0][twice] == 0).all()
    assert (nm[0][~twice] > 0).any()
    for k in range(1024):
        assert np.isfinite(m[0, k, :nm[0, k]]).all()


# ---- input layout -------------------------------------------------------------------------------------------------------
def test_input_layouts_give_identical_results():
    p2d, p3d, _, K = cases.scene("n65")
    wide = np.zeros((65, 7))
    wide[:, 1:3], wide[:, 4:7] = p2d, p3d
    v2, v3 = wide[:, 1:3], wide[:, 4:7]
    assert not v2.flags.c_contiguous and not v3.flags.c_contiguous
    t2, t3 = torch.from_numpy(wide)[:, 1:3], torch.from_numpy(wide)[:, 4:7]
    assert not t2.is_contiguous()
    layouts = {"contiguous float64": (np.ascontiguousarray(p2d, np.float64), np.ascontiguousarray(p3d, np.float64)),
               "strided numpy view": (v2, v3),
               "strided tensor view": (t2, t3),
               "strided device view": (t2.to(DEV), torch.from_numpy(wide).to(DEV)[:, 4:7]),
               "device tensor": (torch.from_numpy(p2d.copy()).to(DEV), torch.from_numpy(p3d.copy()).to(DEV))}
    want = _bits(_solve_case("n65"))
    for what, (a, b) in layouts.items():
        assert _bits(P.estimate_absolute_pose(a, b, K, seed=cases.SEED)) == want, what
    _assert_matches_reference(P.estimate_absolute_pose(v2, v3, torch.from_numpy(K).to(DEV), seed=cases.SEED),
                              cases.reference("n65"), "n65 strided")
