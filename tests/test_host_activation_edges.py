"""Host side of the activation-stage edge tests (tests/test_gpu_activation_edges.py): every named case of
tests/activation_reference.py reaches the edge it is named for, the float32 model of the two kernels (`model32`) and of the statistics
kernel (`stats_model`) meets every check the device tests make, each deliberate defect fails the check named for it, a planted NaN or
infinity fails the bars, torch's own CPU float32 path lies inside them, the torch restatement equals what the reference's own code
recorded in tests/golden/activation_edges.npz, and the C entry points refuse bad arguments before any launch.  No GPU needed.

Measured with the model, worst |model - float64| / bar over the cases: scales 0.69, rotations 0.21, opacities 0.31, colours 0.23,
d_xyz 0.033, d_f_dc 0.93 (two roundings: the constant and the product), d_f_rest 0.17, d_scaling 0.39, d_rotation 0.11, d_opacity
0.16; with torch's CPU float32 path every ratio is below 0.5 as well."""
import ctypes
import os

import numpy as np
import pytest

from tests import activation_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "activation_edges.npz")
QUAD_CASES = [n for n in R.CASES if n.startswith("cw")]
STATS_SHAPES = [(P, V) for V in (1, 2, 8) for P in (1, 255, 256, 257)]


def _quad_crosses_a_row(P, CW):
    return any((4 * t) % CW + 3 >= CW and (4 * t) // CW + 1 < P for t in range((P * CW + 3) // 4))


def test_every_case_reaches_the_edge_it_is_named_for():
    cases = {n: R.case(n) for n in R.CASES}
    assert all(c["edge"] and c["name"] == n for n, c in cases.items())
    counts = {n: R.item_count(c["P"], 3 + c["E"]) for n, c in cases.items()}
    for cw in (3, 4, 5, 8, 35):
        got = sorted(counts[n] for n in QUAD_CASES if n.startswith(f"cw{cw}_"))
        assert got and all(254 <= k <= 263 for k in got), (cw, got)
    assert {255, 256, 257} <= {counts[n] for n in QUAD_CASES}
    assert [counts["cw5_p204_deg2"], counts["cw5_p205_deg0"], counts["cw8_p128_deg0of3"]] == [255, 257, 256]
    assert [counts["cw35_p29_deg1"], counts["cw35_p30_deg0"]] == [254, 263]             # no P gives 255 .. 257 at CW = 35
    assert not any(254 < R.item_count(P, 35) < 263 for P in range(1, 100))
    assert {c["P"] for c in cases.values()} >= {1, 2, 3, 5}
    assert {c["P"] * (3 + c["E"]) % 4 for c in cases.values()} == {0, 1, 2, 3}           # every tail length
    assert {c["P"] * (3 + c["E"]) % 4 for n, c in cases.items() if n in QUAD_CASES} == {0, 1, 2, 3}
    for n in QUAD_CASES:
        c = cases[n]
        CW, quads = 3 + c["E"], (c["P"] * (3 + c["E"]) + 3) // 4
        assert _quad_crosses_a_row(c["P"], CW) == (CW % 4 != 0), n                        # CW = 4: a quad is exactly one row; 8: two quads
        assert (quads < c["P"]) == (c["E"] == 0) and (quads > c["P"]) == (c["E"] >= 2), n
    assert {(c["deg"], c["K"]) for c in cases.values()} >= {(0, 1), (1, 4), (2, 9), (3, 16), (0, 16), (1, 16), (2, 16)}
    assert {c["SC"] for c in cases.values()} == {1, 3} and {c["SC"] for c in cases.values() if c["deg"] > 0} == {1, 3}
    # the clamp: degree 0 at raw == 0 exactly and one ulp of f_dc to either side, in every channel
    c = cases["clamp0"]
    raw = (np.float32(R.C0) * c["f_dc"][:, 0, :]).astype(np.float32) + np.float32(0.5)
    for ch in range(3):
        assert sorted(set(raw[:, ch].tolist())) == [-5.960464477539063e-08, 0.0, 2.9802322387695312e-08]
    # degree > 0: planted rows within the forward bar of 0 on both sides, all found by `near`, under the cap
    planted = 0
    for n in QUAD_CASES:
        c, ref = cases[n], R.reference_of(n)
        assert R.near_rows(n) <= R.NEAR_CAP * c["P"], n
        if c["deg"] > 0 and int(R.NEAR_CAP * c["P"]) >= 4:
            rows = int(R.NEAR_CAP * c["P"]) - 2
            vals = np.array([ref["raw"][i, i % 3] for i in range(rows)])
            assert (np.abs(vals) < 4e-7).all() and (vals > 0).any() and (vals < 0).any(), n
            assert all(ref["near"][i, i % 3] for i in range(rows)), n
            planted += rows
    assert planted >= 30
    # saturation and eps rows
    for n in ("saturation_deg0", "saturation_deg2"):
        c = cases[n]
        lo = set(c["opacity"].ravel().tolist())
        assert {20.0, -20.0, 88.0, -88.0, 90.0, -90.0, np.inf, -np.inf} <= lo
        with np.errstate(over="ignore"):
            s = np.exp(c["scaling"].astype(np.float64)).astype(np.float32)
        big = np.isfinite(s) & (s > 1e38)
        assert np.isinf(s).any() and big.any() and (s == 0).any() and ((s > 0) & (s < 2e-38)).any()
        assert float(c["scaling"][np.isinf(s)].min()) < 88.73 and float(c["scaling"][big].max()) > 88.69    # next to the overflow
        nrm = np.sqrt((c["rotation"].astype(np.float64) ** 2).sum(1))
        assert (nrm == 0).any() and ((nrm > 0.98e-12) & (nrm < 1e-12)).any() and ((nrm > 1e-12) & (nrm < 1.02e-12)).any()
        assert nrm.min() == 0 and nrm.max() > 0.9e6 and ((nrm > 0.9e-6) & (nrm < 1.1e-6)).any()
        assert np.array_equal(c["rotation"][13], np.array([3e-14, 4e-14, 0, 0], np.float32))
        assert (c["rotation"][13].astype(np.float32) ** 2)[0] > np.finfo(np.float32).tiny       # the squares are normal numbers
    # one-hot rows: one coefficient, 14 directions, every channel passing
    for deg in (0, 1, 2, 3):
        n = f"onehot_deg{deg}"
        c, ref = cases[n], R.reference_of(n)
        feats = np.concatenate([c["f_dc"], c["f_rest"]], axis=1)
        assert c["K"] == 16 and ((feats != 0).any(2).sum(1) == 1).all() and set(np.nonzero((feats != 0).any(2))[1].tolist()) == set(range(16))
        d = (c["xyz"] - c["campos"]).astype(np.float64)
        assert len({tuple(np.round(v / np.abs(v).max()).tolist()) for v in d}) == 14
        assert ref["passing"].all() and not ref["near"].any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_model_meets_every_check(name):
    got = {}

    def run(c):
        got.update(R.model32(c))
        return got

    ratios = R.check_bounded(run, name)
    assert R.within(ratios), (name, ratios)
    assert R.check_exact(got, name) == [] and R.check_consistency(got, name) == [] and not got["past_end"], name
    for k in R.FORWARD + R.BACKWARD:
        assert got[k] is None or got[k].dtype == np.float32


def _fails(wrong):
    _what, name, check = R.WRONG[wrong]
    if check == "stats":
        return any(R.check_stats(lambda g, r, a, d, m, s=R.stats_case(P, V): R.stats_model(
            dict(s, accum=a if a is not None else s["accum"], denom=d if d is not None else s["denom"], max_radii=m),
            only_max=a is None, wrong=wrong), P, V) for P, V in STATS_SHAPES)
    out = R.model32(R.case(name), wrong)
    if check == "past_end":
        return out["past_end"]
    if check == "exact":
        return R.check_exact(out, name) != []
    if check == "consistency":
        return R.check_consistency(out, name) != []
    return not R.within(R.check_bounded(lambda c: out, name))


@pytest.mark.parametrize("wrong", list(R.WRONG))
def test_each_defect_fails_the_check_named_for_it(wrong):
    assert _fails(wrong), R.WRONG[wrong]


def test_defect_list_is_the_issues():
    assert len(R.WRONG) == 19 and {c for _, _, c in R.WRONG.values()} == {"bounded", "past_end", "exact", "consistency", "stats"}


@pytest.mark.parametrize("P,V", STATS_SHAPES)
def test_statistics_model_and_case(P, V):
    s = R.stats_case(P, V)
    for g in s["grads"]:
        x, y = g[:, 0].astype(np.float64), g[:, 1].astype(np.float64)
        root = np.sqrt(x * x + y * y)
        assert np.isnan(g[:, 2]).all() and np.array_equal(root, root.astype(np.float32)) and np.array_equal(x * x + y * y, (x * x + y * y).astype(np.float32))
    if P >= 255:
        assert (~s["seen"]).sum() >= P // 8 and any((r < 0).any() and (r == 0).any() for r in s["radii"])
        assert np.isnan(s["accum"][~s["seen"]]).any() and np.signbit(s["max_radii"][~s["seen"]]).any()
        if V >= 2:          # the running sum rounds: the order matters
            assert not R.same_bits(R.stats_model(s)[0], R.stats_model(s, wrong="stats_reverse")[0])
    assert R.check_stats(lambda g, r, a, d, m: R.stats_model(dict(s, accum=a if a is not None else s["accum"],
                                                                    denom=d if d is not None else s["denom"], max_radii=m), only_max=a is None), P, V) == []


@pytest.mark.parametrize("name", ["cw4_p256_deg3", "saturation_deg0"])
def test_planted_nan_or_infinity_fails_the_bars(name):
    c, ref = R.case(name), R.reference_of(name)
    for k in ("scales", "colors", "d_rotation", "d_f_dc", "d_opacity"):
        for bad in (np.nan, np.inf, -np.inf):
            out = R.model32(c)
            flat = out[k].reshape(-1)
            with np.errstate(over="ignore"):
                i = int(np.flatnonzero(np.isfinite(ref[k].astype(np.float32).reshape(-1)))[5])
            flat[i] = bad
            r = R.check_bounded(lambda c_: out, name)
            assert r[k] == float("inf") or (k == "d_f_dc" and r["clamp"] == float("inf")), (name, k, bad, r)
    if name == "saturation_deg0":       # and where the reference has an infinity the device must have the same one
        out = R.model32(c)
        i = int(np.flatnonzero(np.isinf(out["scales"].reshape(-1)))[0])
        for bad in (np.nan, -np.inf, np.float32(3e38)):
            out["scales"].reshape(-1)[i] = bad
            assert R.check_bounded(lambda c_: out, name)["scales"] == float("inf")
    assert R.worst(np.zeros(3), np.zeros(3), np.zeros(3)) == 0.0 and R.worst(np.array([1e-30]), np.zeros(1), np.zeros(1)) == float("inf")
    assert not R.within({"a": float("nan")})


@pytest.mark.parametrize("name", list(R.CASES))
def test_torch_cpu_float32_lies_inside_the_bars(name):
    ratios = R.check_bounded(R.torch32, name)
    assert R.within(ratios), (name, ratios)


def test_measured_roundings_are_what_the_module_says():
    E, S, D = R.measured_roundings()
    # four times one rounding where the CPU rounds correctly (measured here: 3.96, 4.09, 3.96), at most four times one ulp
    assert 2.0 <= S <= 8.5 and 2.0 <= D <= 8.5 and 2.0 <= E <= 16.0, (E, S, D)
    assert R.roundings(0)["d_extra"] == 0 and R.roundings(3)["colors"] > R.roundings(1)["colors"]


def test_restatement_equals_the_reference_code_fixture():
    assert os.path.getsize(GOLD) < 1_000_000
    d = np.load(GOLD, allow_pickle=False)
    assert all(d[k].dtype.kind in "fiu" for k in d.files) and len(d.files) > 50
    assert d["clamp_rule"].tolist() == [1.0, 1.0, 1.0, 0.0]                              # passes at +0, -0 and 1e-30, blocks at -1e-30
    for tag in ("f32", "f64"):
        assert np.allclose(d["normalize_sub_eps_" + tag], np.array([[1e12, 2e12, 3e12, 4e12]]), rtol=1e-6, atol=0)
    names = sorted({k.split("__")[0] for k in d.files if "__" in k})
    assert len(names) == 9 and "onehot_deg3" in names and "saturation_deg0" in names
    for name in names:
        c, ref = R.case(name), R.reference_of(name)
        for k in R.FORWARD + R.BACKWARD:
            if k == "d_extra" and not c["E"]:
                continue
            gold = d[f"{name}__{k}"].reshape(ref[k].shape)
            keep = np.isfinite(ref[k]) & np.isfinite(gold) if k == "d_scaling" else np.ones(gold.shape, bool)
            with np.errstate(invalid="ignore"):
                err = np.abs(ref[k] - gold)
            assert (err[keep] <= 1e-12 * ref["terms"][k][keep] + 1e-300).all(), (name, k, float(err[keep].max()))
    # the oracle's hand-derived backward and the float32 model follow the same rule on that row
    from oracle import activations as act
    c = R.case("saturation_deg0")
    g = act.backward(c["xyz"], c["f_dc"], c["f_rest"], c["scaling"], c["rotation"], c["opacity"], c["extra"], c["campos"], 0,
                     c["G_scales"], c["G_rotations"], c["G_opacities"], c["G_colors"])
    assert np.array_equal(g["d_rotation"][13], np.array([1e12, 2e12, 3e12, 4e12]))
    assert np.allclose(R.model32(c)["d_rotation"][13], [1e12, 2e12, 3e12, 4e12], rtol=2e-7, atol=0)
    ref = R.reference_of("saturation_deg0")
    assert np.allclose(ref["d_rotation"][[10, 11, 13, 14]], c["G_rotations"][[10, 11, 13, 14]].astype(np.float64) / 1e-12, rtol=1e-15)


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below fails validation, so none reaches a launch (the pointers are host addresses that are never read)."""
    from splatloc_amd import _native
    lib = _native.load()
    buf = ctypes.create_string_buffer(64)
    A = ctypes.c_void_p(ctypes.addressof(buf))
    BAD, UNSUPPORTED = 1, _native.ERR_UNSUPPORTED
    fwd, bwd = lib.splatraster_activate_forward, lib.splatraster_activate_backward

    def both(P, K, deg, SC, E, f_rest=A, extra=A, campos=A):
        a = fwd(P, K, deg, SC, E, A, A, f_rest, A, A, A, extra, campos, A, A, A, A, None)
        b = bwd(P, K, deg, SC, E, A, A, f_rest, A, A, A, campos, A, A, A, A, A, A, A, A, A, A, extra, None)
        assert a == b, (a, b)
        return a

    assert both(10, 25, 4, 3, 1) == UNSUPPORTED                # SH degree 4
    assert both(10, 16, 7, 3, 1) == UNSUPPORTED
    assert both(10, 1, 1, 3, 1) == BAD and both(10, 8, 2, 3, 1) == BAD and both(10, 15, 3, 3, 1) == BAD      # (deg + 1)^2 > K
    assert both(10, 1, 0, 2, 1) == BAD and both(10, 1, 0, 0, 1) == BAD and both(10, 1, 0, 4, 1) == BAD        # SC not in {1, 3}
    assert both(10, 4, 1, 3, 1, f_rest=None) == BAD            # K > 1 without f_rest
    assert both(10, 1, 0, 3, 2, extra=None) == BAD             # E > 0 without extra / dL_dextra
    assert both(10, 4, 1, 3, 1, campos=None) == BAD            # degree > 0 without the camera centre
    assert both(-1, 1, 0, 3, 0) == BAD and both(10, 0, 0, 3, 0) == BAD and both(10, 1, -1, 3, 0) == BAD and both(10, 1, 0, 3, -1) == BAD
    assert bwd(10, 4, 1, 3, 0, A, A, A, A, A, A, A, A, A, A, A, A, A, None, A, A, A, None, None) == BAD       # K > 1 without dL_df_rest
    assert both(0, 1, 0, 3, 0, None, None, None) == 0          # an empty model needs no pointers
    win = lib.splatraster_densification_stats_window
    ptrs = (ctypes.c_void_p * 9)(*[A.value] * 9)
    assert win(10, _native.MAX_WINDOW_VIEWS + 1, ptrs, ptrs, A, A, A, None) == BAD
    assert win(10, -1, ptrs, ptrs, A, A, A, None) == BAD and win(-1, 1, ptrs, ptrs, A, A, A, None) == BAD
    assert win(10, 2, ptrs, ptrs, A, None, A, None) == BAD and win(10, 2, ptrs, ptrs, None, A, A, None) == BAD   # accum xor denom
    assert win(10, 2, None, ptrs, A, A, A, None) == BAD        # statistics asked for without gradients
    assert win(10, 2, ptrs, None, A, A, A, None) == BAD and win(10, 2, ptrs, ptrs, A, A, None, None) == BAD
    hole = (ctypes.c_void_p * 2)(A.value, None)
    assert win(10, 2, ptrs, hole, A, A, A, None) == BAD and win(10, 2, hole, ptrs, A, A, A, None) == BAD
    assert win(0, 2, None, None, None, None, None, None) == 0 and win(10, 0, None, None, None, None, None, None) == 0
    assert lib.splatraster_densification_stats(10, A, A, A, None, A, None) == BAD
