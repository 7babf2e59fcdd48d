"""tests/model_update_reference.py pinned on the host: the seeded builders reproduce the inputs tests/golden/model_update_edges.npz was
recorded from, the restatements reproduce what the reference's own GaussianModel.densify_and_prune / extend_from_pcd left (which pins
oracle/densify.py's tie rules, the double-product thresholds included, to the reference's), every case reaches the edge it is named for,
every wrong model leaves the bound (or the exact result) on a named case, and torch's CPU float32 Adam lies inside the Adam bound.  The
argument checks of the stage's C entry points run here too: they return before any HIP call.  No test here touches a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import model_update_reference as R

F32, F64 = np.float32, np.float64
GOLD = os.path.join(os.path.dirname(__file__), "golden", "model_update_edges.npz")
G = R.GROUPS


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def dens():
    """every densify case with the oracle's result, computed once"""
    out = {}
    for name in R.densify_case_names():
        c = R.densify_case(name)
        out[name] = (c,) + tuple(R.densify_oracle(c))
    return out


def _kinds_of(src, kind, row):
    return sorted(int(k) for k in kind[src == row])


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_builders_reproduce_the_recorded_inputs(gold, dens):
    for name, (c, *_) in dens.items():
        assert np.array_equal(R.checksum(*R.densify_inputs(c)), gold[f"densify__{name}__checksum"]), name
    for name in R.append_case_names():
        assert np.array_equal(R.checksum(*R.append_inputs(R.append_case(name))), gold[f"append__{name}__checksum"]), name
    assert not any("stride" in k for k in gold.files)                # oracle only
    assert os.path.getsize(GOLD) < 1_000_000
    assert all(gold[k].dtype.kind in "fu" for k in gold.files)       # data only


@pytest.mark.parametrize("name", R.densify_case_names())
def test_densify_restatement_reproduces_the_reference(gold, dens, name):
    c, p, st, src, kind = dens[name]
    pre = f"densify__{name}__"
    assert p["xyz"].shape[0] == int(gold[pre + "rows"][0]) == src.size == kind.size
    m = {k: s["m"] for k, s in st.items()} or None
    v = {k: s["v"] for k, s in st.items()} or None
    assert np.array_equal(R.outputs_checksum(p, m, v), gold[pre + "copied"])       # row order, copies, moments: exact
    assert gold[pre + "steps"].size == (7 if c["m"] is not None else 0) and (gold[pre + "steps"] == c["step"]).all()
    x64, xb, s64, sb = R.densify_split_f64(c, src, kind)
    for got_x, got_s in ((gold[pre + "xyz"], gold[pre + "scaling"]), (p["xyz"], p["scaling"])):   # the reference, the float32 oracle
        assert got_x.shape == x64.shape and got_s.shape == s64.shape
        assert not R.exceeds(np.abs(got_x - x64), xb).any() and not R.exceeds(np.abs(got_s - s64), sb).any()
    # the rules written on the kernel's four sections give the same rows
    msrc, mkind = R.densify_plan_model(c)
    assert np.array_equal(msrc, src) and np.array_equal(mkind, kind)
    # copies: exactly the source rows; moments: originals keep theirs, every new row zero
    for k in G:
        if k not in ("xyz", "scaling"):
            assert np.array_equal(p[k], c["params"][k][src]), k
    assert np.array_equal(p["xyz"][kind < 2], c["params"]["xyz"][src[kind < 2]])
    for k in st:
        assert np.array_equal(st[k]["m"], np.where((kind == 0).reshape((-1,) + (1,) * (c["m"][k].ndim - 1)), c["m"][k][src], 0)), k
    assert "marker" not in st


@pytest.mark.parametrize("name", R.append_case_names())
def test_append_restatement_reproduces_the_reference(gold, name):
    c = R.append_case(name)
    p, m, v = R.append_expected(c)
    pre = f"append__{name}__"
    assert p["xyz"].shape[0] == int(gold[pre + "rows"][0]) == c["P"] + c["N"]
    arrs = [p[k] for k in G] + ([] if m is None else [m[k] for k in G if k in m] + [v[k] for k in G if k in v])
    assert np.array_equal(R.checksum(*arrs), gold[pre + "all"])
    assert gold[pre + "steps"].size == (7 if m is not None else 0) and (gold[pre + "steps"] == c["step"]).all()


# ---- every case reaches its edge ---------------------------------------------------------------------------------------------------
def test_threshold_hypers_are_what_they_are_named_for():
    one = F32(1)
    want = {"tie": (one, one), "below": (R.below(one), one), "above": (R.above(one), one)}
    for h, (ref, flt) in want.items():
        pd, ext, ln_split, ln_prune = R.HYPERS[h]
        assert float(F32(ext)) == ext                                 # float32-exact extents
        assert R.thresholds(pd, ext)[0] == ref and R.thresholds_float_products(pd, ext)[0] == flt, h
        assert ln_split == 0.0 and abs(ln_prune - np.log(float(R.thresholds(pd, ext)[1]))) < 1e-6
    pd, ext, ln_split, ln_prune = R.HYPERS["tenth"]
    assert ext == float(F32(0.01 * 110))                              # an extent of the form 0.01 m
    assert R.thresholds(pd, ext)[1] != R.thresholds_float_products(pd, ext)[1]
    assert R.thresholds(pd, ext)[0] == R.thresholds_float_products(pd, ext)[0]
    assert abs(ln_split - np.log(float(R.thresholds(pd, ext)[0]))) < 1e-6 and abs(ln_prune - np.log(float(R.thresholds(pd, ext)[1]))) < 1e-6
    differing = sum(R.thresholds(0.01, float(F32(0.01 * m)))[1] != R.thresholds_float_products(0.01, float(F32(0.01 * m)))[1]
                    for m in range(100, 3000))
    assert differing >= 200


def test_densify_cases_keep_their_margin_and_redraw_cap(dens):
    Ps, scs, frs, kps, moms = set(), set(), set(), set(), set()
    for name, (c, p, st, src, kind) in dens.items():
        assert c["redraws"] <= R.REDRAW_CAP and R.densify_margin_ok(c), name
        par = c["params"]
        Ps.add(par["xyz"].shape[0]); scs.add(par["scaling"].shape[1]); kps.add(par["kp_score"].shape[1])
        frs.add(par["f_rest"].shape[1] * 3); moms.add(c["m"] is not None)
        assert c["m"] is None or "marker" not in c["m"]
        q = par["rotation"].astype(F64)
        assert (np.sqrt((q * q).sum(1)) > 0.5).all()
    assert Ps >= {1, 2, 255, 256, 257, 1025} and scs == {1, 3} and frs == {0, 9, 45} and kps == {1, 2} and moms == {True, False}
    # the generic models take every branch
    c, p, st, src, kind = dens[R.width_name(R.WIDTH_CASES[-1])]
    assert set(kind.tolist()) == {0, 1, 2, 3} and src.size not in (0, c["accum"].size)


def test_tie_rows_sit_on_their_ties(dens):
    mg = F32(R.MAX_GRAD)
    c, p, st, src, kind = dens["tie grad"]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = c["accum"][:, 0] / c["denom"][:, 0]
    for suffix in ("", " (end)"):
        r = lambda lab: c["rows"][lab + suffix]  # noqa: E731
        assert g[r("quotient small")] == mg and g[r("at large")] == mg and g[r("below small")] == R.below(mg) and g[r("above large")] == R.above(mg)
        assert np.isnan(g[r("nan small")]) and g[r("inf large")] == np.inf and g[r("neg inf small")] == -np.inf and g[r("neg at small")] == -mg
        for lab in ("quotient", "at", "above", "inf"):
            assert _kinds_of(src, kind, r(lab + " small")) == [0, 1] and _kinds_of(src, kind, r(lab + " large")) == [2, 3], lab
        for lab in ("below", "nan", "neg below", "neg zero"):
            assert _kinds_of(src, kind, r(lab + " small")) == [0] and _kinds_of(src, kind, r(lab + " large")) == [0], lab
        for lab in ("neg at", "neg inf"):      # |g| clones, the padded gradient itself never splits
            assert _kinds_of(src, kind, r(lab + " small")) == [0, 1] and _kinds_of(src, kind, r(lab + " large")) == [0], lab
    assert c["rows"]["neg zero large (end)"] == 256                  # the last planted row is alone in the flag kernel's second block
    # scale: exp(0) == 1 sits on size_split = 1 (clone), above 1 - 2^-24 (split), below 1 + 2^-23 (clone)
    for name, want in (("tie scale below", [2, 3]), ("tie scale at", [0, 1]), ("tie scale above", [0, 1])):
        c, p, st, src, kind = dens[name]
        for lab in ("all", "first", "last"):
            row = c["rows"]["hot " + lab]
            assert c["params"]["scaling"][row].max() == 0 and np.exp(c["params"]["scaling"][row]).astype(F32).max() == 1
            assert _kinds_of(src, kind, row) == want and _kinds_of(src, kind, c["rows"]["cold " + lab]) == [0], (name, lab)
    # opacity: sigmoid(0) == 0.5
    for name, pruned in (("tie opacity below", False), ("tie opacity at", False), ("tie opacity above", True)):
        c, p, st, src, kind = dens[name]
        row = c["rows"]["cold"]
        assert c["params"]["opacity"][row, 0] == 0 and F32(1) / (F32(1) + np.exp(F32(-0.0))) == F32(0.5)
        assert _kinds_of(src, kind, row) == ([] if pruned else [0])
        assert _kinds_of(src, kind, c["rows"]["clone"]) == ([] if pruned else [0, 1])
        assert _kinds_of(src, kind, c["rows"]["split"]) == ([] if pruned else [2, 3])
    # marker: <= 0.005f opens the prune
    c, p, st, src, kind = dens["tie marker"]
    assert c["params"]["marker"][c["rows"]["at cold"], 0] == R.MARKER_THR
    for lab, pruned in (("at", True), ("below", True), ("zero", True), ("above", False), ("key", False)):
        assert _kinds_of(src, kind, c["rows"][lab + " cold"]) == ([] if pruned else [0]), lab
        assert _kinds_of(src, kind, c["rows"][lab + " clone"]) == ([] if pruned else [0, 1]), lab
        assert _kinds_of(src, kind, c["rows"][lab + " split"]) == ([] if pruned else [2, 3]), lab


def test_outcome_cases_end_as_named(dens):
    c, p, st, src, kind = dens["outcome none"]
    assert all(np.array_equal(p[k], c["params"][k]) for k in G) and all(np.array_equal(st[k]["m"], c["m"][k]) for k in st)
    assert np.array_equal(src, np.arange(6)) and not kind.any()
    assert dens["outcome all cloned"][4].tolist() == [0] * 6 + [1] * 6
    assert dens["outcome all split kept"][4].tolist() == [2] * 6 + [3] * 6
    for name in ("outcome all split pruned", "outcome all pruned"):
        c, p, st, src, kind = dens[name]
        assert src.size == 0 and all(p[k].shape == (0,) + c["params"][k].shape[1:] for k in G)
    c, p, st, src, kind = dens["outcome parent size"]
    r = c["rows"]
    assert _kinds_of(src, kind, r["hot over"]) == [2, 3] and _kinds_of(src, kind, r["cold over"]) == []
    assert _kinds_of(src, kind, r["hot far over"]) == [] and _kinds_of(src, kind, r["cold under"]) == [0]
    assert _kinds_of(src, kind, r["hot under"]) == [2, 3] and _kinds_of(src, kind, r["cold small"]) == [0]
    c, p, st, src, kind = dens["outcome key primitives"]
    assert sorted(set(src.tolist())) == [0, 1, 2, 3] and set(kind.tolist()) == {0, 1, 2, 3}    # rows 4, 5 (marker 0) are pruned


def test_stride_and_size_cases_exceed_the_first_grid_pass():
    q = R.adam_stride_case("quads")["groups"][0]["p"].size
    assert q // 4 == R.ADAM_QUAD_CAP + 1 and q % 4 == 1                # 1,048,577 full quads and a partial one
    assert R.adam_stride_case("elements")["groups"][0]["p"].size == R.ADAM_QUAD_CAP + 1
    assert (R.STRIDE_RADII + 3) // 4 > 1
    assert max(P for _, P in R.ISO_CASES) > R.ISO_ROW_CAP and any(-(-P // R.ISO_BLOCK) > 64 for _, P in R.ISO_CASES)
    assert {V for V, _, _ in R.STATS_CASES} == {1, 2, 8, 9} and R.MAX_WINDOW_VIEWS == 8
    for V, P, om in R.STATS_CASES:
        c = R.stats_case(V, P, om)
        pats = {tuple(col) for col in c["sees"].T}
        assert len(pats) == min(P, 1 << V) and (c["radii"][~c["sees"]] <= 0).all() and (c["radii"][c["sees"]] > 0).all()
        if P > 1:
            assert (c["radii"] < 0).any() and (c["radii"] == 0).any()
    c = R.stats_case(2, 255, False)
    unseen = ~c["sees"].any(0)
    for k in ("accum", "denom", "max_radii"):       # rows no view sees start as NaN, -0.0 and inf in each of the three vectors
        u = c[k][unseen]
        assert unseen.sum() > 3 and np.isnan(u).any() and np.isinf(u).any() and (np.signbit(u) & (u == 0)).any()
    assert (~R.stats_case(8, 257, False)["sees"].any(0)).sum() == 1


def test_adam_cases_reach_their_regimes():
    names = R.adam_case_names()
    for mag in R.MAGNITUDES:
        for step in R.STEPS:
            assert f"{mag} step {step}" in names
    c = R.adam_case("eps step 1")
    r = R.adam_f64(c["groups"][0])
    s = np.sqrt(r["v"]) / np.sqrt(1 - R.BETA2)
    assert ((s < 10 * R.EPS) & (s > 0.01 * R.EPS)).any()                                  # eps decides the step
    c = R.adam_case("subnormal step 2")
    r = R.adam_f64(c["groups"][0])
    tiny = float(np.finfo(F32).tiny)
    assert (c["groups"][0]["v"] < tiny).all() and ((r["v"] < tiny) & (r["v"] > 0)).all()  # v stays subnormal
    c = R.adam_case("mixed step 1000")
    assert (np.abs(c["groups"][0]["m"]) > 100 * np.abs(c["groups"][0]["g"])).any() and (c["groups"][0]["m"] * c["groups"][0]["g"] < 0).any()
    c = R.adam_case("gate")
    vals = c["gate"][0][:, 0]
    thr = F32(R.GATE_THR)
    assert vals[0] == thr and vals[1] == R.above(thr) and vals[2] == R.below(thr) and np.isnan(vals[3])
    for P in (1, 2, 3, 5):
        c = R.adam_case(f"model P{P}")
        assert [g["name"] for g in c["groups"]] == list(G) and c["groups"][2]["p"].size == 0 and c["groups"][4]["g"] is None
        assert all(g["p"].size <= 4 * P for g in c["groups"])
        assert R.adam_f64(c["groups"][2]) is None and R.adam_f64(c["groups"][4]) is None       # skipped groups get no state
    c = R.adam_case("widths")
    assert [g["p"].shape[1] for g in c["groups"]] == [1, 3, 5, 4, 9] and c["groups"][2]["g"] is None


# ---- wrong models ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong,name", [("grad_gt", "tie grad"), ("split_abs_grad", "tie grad"), ("size_lt", "tie scale at"),
                                        ("opacity_le", "tie opacity at"), ("float_products", "tie scale below"),
                                        ("child_parent_size", "outcome parent size"), ("marker_lt", "tie marker")])
def test_wrong_densify_rules_change_the_rows(dens, wrong, name):
    assert wrong in R.DENSIFY_WRONG
    c, p, st, src, kind = dens[name]
    wsrc, wkind = R.densify_plan_model(c, wrong)
    assert not (np.array_equal(wsrc, src) and np.array_equal(wkind, kind))
    if wrong == "float_products":            # the fault the stage had: the hot row on exp(0) = 1 is cloned, the reference splits it
        row = c["rows"]["hot all"]
        assert _kinds_of(wsrc, wkind, row) == [0, 1] and _kinds_of(src, kind, row) == [2, 3]


def test_wrong_densify_values_leave_the_result(dens):
    name = R.width_name(R.WIDTH_CASES[4])
    c, p, st, src, kind = dens[name]
    wp, wst = R.densify_values_wrong(c, p, st, src, kind, "clone_moments")
    assert (kind == 1).any() and any(not np.array_equal(wst[k]["m"], st[k]["m"]) for k in st)
    wp, wst = R.densify_values_wrong(c, p, st, src, kind, "child_scale")
    x64, xb, s64, sb = R.densify_split_f64(c, src, kind)
    assert R.exceeds(np.abs(wp["scaling"] - s64), sb)[kind >= 2].all()


def test_wrong_philox_models_leave_the_draw_bound():
    rows = np.array([0, 1, 256])
    for seed in R.DRAW_WORDS:
        for did in R.DRAW_WORDS:
            z, b = R.normal3(seed, did, rows, 1)
            assert np.isfinite(z).all()
            for wrong, word in (("no_k1", seed), ("no_ctr_hi", did)):
                w, _ = R.normal3(seed, did, rows, 1, wrong)
                assert np.array_equal(w, z) == (word < 2 ** 32), (wrong, seed, did)
                if word >= 2 ** 32:
                    assert R.exceeds(np.abs(w - z), b).any()
    # known answer of Philox4x32-10 (Random123 kat_vectors): zero counter and key
    assert R.philox4x32(0, np.array([0], np.uint64), 0)[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFFFFFFFFFF
    assert R.philox4x32(ones, np.array([ones], np.uint64), ones)[0].tolist() == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def _adam_within(got, ref):
    return max(R.worst_ratio(got[k], ref[k], ref["b" + k]) for k in "pmv")


@pytest.mark.parametrize("wrong,name", [("eps_before_bc", "eps step 1"), ("beta_for_omb", "ordinary step 2"),
                                        ("gate_per_element", "gate")])
def test_wrong_adam_models_leave_the_bound(wrong, name):
    assert wrong in R.ADAM_WRONG
    c = R.adam_case(name)
    grp = c["groups"][0]
    ref, bad = R.adam_f64(grp, c["gate"]), R.adam_f64(grp, c["gate"], wrong)
    assert _adam_within(bad, ref) > 1.0


def test_wrong_statistics_and_isotropic_models_fail():
    c = R.stats_case(9, 257, False)
    a, b, n, mx = R.stats_f64(c)
    wa, _, wn, wmx = R.stats_f64(c, "count_unseen")
    assert not np.array_equal(n, wn, equal_nan=True) and R.exceeds(np.abs(wa - a), b).any()
    ic = R.iso_case(3, 5)
    loss, lb, grad, gb, ok = R.iso_f64(ic)
    wl, _, wg, _, _ = R.iso_f64(ic, "mask_ge")
    assert ok and R.exceeds(abs(wl - loss), lb) and R.exceeds(np.abs(wg - grad), gb).any()
    for SC, P in R.ISO_CASES:
        assert R.iso_f64(R.iso_case(SC, P))[4]
    assert R.iso_f64(R.iso_case(3, 16385, empty=True))[0] == 0.0


# ---- an independent conforming implementation lies inside the Adam bound ------------------------------------------------------------
@pytest.mark.parametrize("name", R.adam_case_names())
def test_torch_cpu_adam_lies_within_the_bound(name):
    c = R.adam_case(name)
    params, groups = [], []
    for grp in c["groups"]:
        p = torch.nn.Parameter(torch.from_numpy(grp["p"].copy()))
        params.append(p)
        groups.append({"params": [p], "lr": grp["lr"], "name": grp["name"]})
    opt = torch.optim.Adam(groups, lr=0.0, eps=R.EPS, betas=(R.BETA1, R.BETA2))
    for p, grp in zip(params, c["groups"]):
        if grp["g"] is not None:
            g = grp["g"].copy()
            if c["gate"] is not None and c["gate"][2] == grp["name"]:
                with np.errstate(invalid="ignore"):
                    g[c["gate"][0][:, 0] > F32(c["gate"][1])] = 0          # train_gaussians.py:231-234
            p.grad = torch.from_numpy(g)
        if grp["step_prev"] is not None:
            opt.state[p] = {"step": torch.tensor(grp["step_prev"]), "exp_avg": torch.from_numpy(grp["m"].copy()),
                            "exp_avg_sq": torch.from_numpy(grp["v"].copy())}
    opt.step()
    worst = 0.0
    for p, grp in zip(params, c["groups"]):
        ref = R.adam_f64(grp, c["gate"])
        if ref is None:
            assert grp["step_prev"] is not None or len(opt.state.get(p, {})) == 0 or grp["p"].size == 0
            continue
        st = opt.state[p]
        assert float(st["step"]) == ref["step"]
        got = dict(p=p.detach().numpy(), m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy())
        worst = max(worst, _adam_within(got, ref))
    print(f"{name}: torch CPU worst |torch - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- argument checks of the C entry points: they return before any device work -------------------------------------------------------
def test_entry_points_reject_bad_arguments_on_the_host():
    from splatloc_amd import _native
    lib = _native.load()
    BAD = 1
    m = _native.Model()
    m.P, m.scaling_width = 0, 3
    n = C.c_int32(-1)
    plan = lib.splatraster_densify_plan_thresholds
    assert plan(None, None, None, 1e-4, 0.5, 1.0, 10.0, 1, 0, None, C.byref(n), None) == BAD
    assert plan(C.byref(m), None, None, 1e-4, 0.5, 1.0, 10.0, 1, 0, None, None, None) == BAD
    assert plan(C.byref(m), None, None, 0.0, 0.5, 1.0, 10.0, 1, 0, None, C.byref(n), None) == BAD      # max_grad must be > 0
    assert plan(C.byref(m), None, None, 1e-4, 0.5, 1.0, 10.0, 1, 0, None, C.byref(n), None) == 0 and n.value == 0   # empty model
    assert lib.splatraster_densify_plan(C.byref(m), None, None, 1e-4, 0.5, 100.0, 0.01, 1, 0, None, C.byref(n), None) == 0
    m.P = 4                                                            # rows but no tensors
    assert plan(C.byref(m), None, None, 1e-4, 0.5, 1.0, 10.0, 1, 0, None, C.byref(n), None) == BAD
    m.P, m.scaling_width = 0, 2
    assert plan(C.byref(m), None, None, 1e-4, 0.5, 1.0, 10.0, 1, 0, None, C.byref(n), None) == BAD
    m.scaling_width = 3
    assert lib.splatraster_densify_apply(None, None, None, None, 0, 0, None, 0, None, None, None, None, None, None) == BAD
    assert lib.splatraster_densify_apply(C.byref(m), None, None, None, 0, 0, None, -1, C.byref(m), None, None, None, None, None) == BAD
    assert lib.splatraster_densify_apply(C.byref(m), None, None, None, 0, 0, None, 0, C.byref(m), None, None, None, None, None) == 0
    e = _native.Model()
    e.P, e.scaling_width = 0, 1
    assert lib.splatraster_model_append(None, None, None, C.byref(e), C.byref(m), None, None, None) == BAD
    assert lib.splatraster_model_append(C.byref(m), None, None, C.byref(e), C.byref(m), None, None, None) == BAD    # widths differ
    assert lib.splatraster_model_append(C.byref(m), C.byref(m), None, C.byref(m), C.byref(m), None, None, None) == BAD
    assert lib.splatraster_model_append(C.byref(m), None, None, C.byref(m), None, None, None, None) == BAD
    arr = (_native.AdamGroup * 17)()
    assert lib.splatraster_adam_step(-1, arr, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    assert lib.splatraster_adam_step(17, arr, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    assert lib.splatraster_adam_step(1, None, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    assert lib.splatraster_adam_step(0, None, 0.9, 0.999, 1e-15, 0.0, None) == 0
    assert lib.splatraster_adam_step(16, arr, 0.9, 0.999, 1e-15, 0.0, None) == 0           # every group without a gradient: skipped
    buf = (C.c_float * 4)()
    arr[0].grad, arr[0].numel, arr[0].row_width, arr[0].step = C.addressof(buf), 4, 1, 1.0     # a gradient but no parameter
    assert lib.splatraster_adam_step(1, arr, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    arr[0].param = arr[0].exp_avg = arr[0].exp_avg_sq = C.addressof(buf)
    arr[0].step = 0.0                                                                       # step counts from 1
    assert lib.splatraster_adam_step(1, arr, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    arr[0].step, arr[0].row_width = 1.0, 0
    assert lib.splatraster_adam_step(1, arr, 0.9, 0.999, 1e-15, 0.0, None) == BAD
    assert lib.splatraster_adam_step_radii(0, None, 0.9, 0.999, 1e-15, 0.0, -1, None, None, None) == BAD
    assert lib.splatraster_adam_step_radii(0, None, 0.9, 0.999, 1e-15, 0.0, 5, None, None, None) == BAD
    assert lib.splatraster_adam_step_radii(0, None, 0.9, 0.999, 1e-15, 0.0, 0, None, None, None) == 0
    assert lib.splatraster_adam_step_gated(0, None, 0.9, 0.999, 1e-15, 0.0, None, None) == BAD
    assert lib.splatraster_adam_step_radii_gated(0, None, 0.9, 0.999, 1e-15, 0.0, 0, None, None, None, None) == BAD
    iso = lib.splatraster_isotropic_loss
    assert iso(-1, 3, None, None, None, C.addressof(buf), C.addressof(buf), None) == BAD
    assert iso(0, 2, None, None, None, C.addressof(buf), C.addressof(buf), None) == BAD
    assert iso(0, 3, None, None, None, None, C.addressof(buf), None) == BAD
    assert iso(4, 3, None, None, None, C.addressof(buf), C.addressof(buf), None) == BAD
    assert lib.splatraster_isotropic_loss_workspace_bytes(0) == 16 and lib.splatraster_isotropic_loss_workspace_bytes(10 ** 6) == 1024 * 16
    win = lib.splatraster_densification_stats_window
    ptrs = (C.c_void_p * 9)()
    assert win(4, R.MAX_WINDOW_VIEWS + 1, ptrs, ptrs, None, None, C.addressof(buf), None) == BAD
    assert win(4, -1, ptrs, ptrs, None, None, C.addressof(buf), None) == BAD
    assert win(4, 1, ptrs, None, None, None, C.addressof(buf), None) == BAD
    assert win(4, 1, ptrs, ptrs, None, None, None, None) == BAD
    assert win(4, 1, ptrs, ptrs, C.addressof(buf), None, C.addressof(buf), None) == BAD     # accum without denom
    assert win(4, 1, ptrs, ptrs, None, None, C.addressof(buf), None) == BAD                # a NULL radii entry
    assert win(0, 1, ptrs, ptrs, None, None, None, None) == 0 and win(4, 0, None, None, None, None, None, None) == 0
    assert lib.splatraster_densify_workspace_bytes(0) == lib.splatraster_densify_workspace_bytes(1) > 0
