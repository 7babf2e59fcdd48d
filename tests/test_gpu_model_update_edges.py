"""The model-update stage on the device at its tie, width and stride edges (cases, float64 restatements and bounds:
tests/model_update_reference.py; the same cases against the reference's own code: tests/test_host_model_update_edges.py).

Exact: row counts, source_row, source_kind, copied groups, moments, untouched rows.  Everything that passes through float32 arithmetic
is compared with the float64 restatement under the bound derived in the reference module; each test prints its worst
|HIP - float64| / bound (recorded in DESIGN.md)."""
import types

import numpy as np
import pytest
import torch

from tests import model_update_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
G = R.GROUPS
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "marker": "_marker", "kp_score": "_kp_score", "scaling": "_scaling", "rotation": "_rotation"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _shifted(t):
    """the same values one float into a larger buffer: 4-byte aligned only (the scalar Adam kernel)"""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 != 0 or t.numel() == 0) and v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def dens():
    out = {}
    for name in R.densify_case_names():
        c = R.densify_case(name)
        out[name] = (c,) + tuple(R.densify_oracle(c))
    return out


def _model(params, m, v, step, adam_cls):
    """a stand-in with the attribute / optimizer layout of the reference's GaussianModel after training_setup"""
    gm = types.SimpleNamespace()
    groups = []
    for k in G:
        p = torch.nn.Parameter(_t(params[k]).requires_grad_(True))
        setattr(gm, ATTR[k], p)
        groups.append({"params": [p], "lr": R.TRAINING_LRS[k], "name": k})
    gm.optimizer = adam_cls(groups, lr=0.0, eps=1e-15)
    if m is not None:
        for grp in gm.optimizer.param_groups:
            if grp["name"] in m:
                gm.optimizer.state[grp["params"][0]] = {"step": torch.tensor(float(step)), "exp_avg": _t(m[grp["name"]]),
                                                        "exp_avg_sq": _t(v[grp["name"]])}
    P = params["xyz"].shape[0]
    gm.xyz_gradient_accum, gm.denom = torch.ones((P, 1), device=DEV), torch.ones((P, 1), device=DEV)
    gm.max_radii2D = torch.ones((P,), device=DEV)
    return gm


def _check_model_object(gm, p_want, m_want, v_want, step, exact_all, bounds=None):
    n = p_want["xyz"].shape[0]
    for k in G:
        got = getattr(gm, ATTR[k])
        assert isinstance(got, torch.nn.Parameter) and got.requires_grad and tuple(got.shape) == p_want[k].shape, k
        if exact_all or k not in ("xyz", "scaling"):
            assert np.array_equal(_n(got), p_want[k]), k
        else:
            want64, bound = bounds[k]
            assert not R.exceeds(np.abs(_n(got) - want64), bound).any(), k
    for grp in gm.optimizer.param_groups:
        k, p = grp["name"], grp["params"][0]
        assert p is getattr(gm, ATTR[k])
        st = gm.optimizer.state.get(p, {})
        if m_want is not None and k in m_want:
            assert np.array_equal(_n(st["exp_avg"]), m_want[k]) and np.array_equal(_n(st["exp_avg_sq"]), v_want[k]), k
            assert float(st["step"]) == step
        else:
            assert len(st) == 0, k
    assert gm.xyz_gradient_accum.shape == (n, 1) and gm.denom.shape == (n, 1) and gm.max_radii2D.shape == (n,)
    assert not gm.xyz_gradient_accum.any() and not gm.denom.any() and not gm.max_radii2D.any()


# ---- densify ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.densify_case_names())
def test_densify_tensors_on_every_case(dens, name):
    from splatloc_amd.densify import densify_tensors
    c, p, st, src, kind = dens[name]
    h = c["hyper"]
    m = {} if c["m"] is None else {k: _t(a) for k, a in c["m"].items()}
    v = {} if c["v"] is None else {k: _t(a) for k, a in c["v"].items()}
    out_p, out_m, out_v, srow, skind = densify_tensors(
        {k: _t(a) for k, a in c["params"].items()}, m, v, _t(c["accum"]), _t(c["denom"]), h["max_grad"], h["min_opacity"],
        h["extent"], h["max_screen_size"], h["percent_dense"], h["primitive_reg"], unit_noise=_t(c["unit_noise"]), return_sources=True)
    assert out_p["xyz"].shape[0] == src.size
    assert np.array_equal(_n(srow), src) and np.array_equal(_n(skind), kind)
    for k in G:
        assert tuple(out_p[k].shape) == p[k].shape, k
        if k not in ("xyz", "scaling"):
            assert np.array_equal(_n(out_p[k]), p[k]), k
    assert set(out_m) == set(st) == set(out_v) and "marker" not in out_m
    for k in st:
        assert np.array_equal(_n(out_m[k]), st[k]["m"]) and np.array_equal(_n(out_v[k]), st[k]["v"]), k
    x64, xb, s64, sb = R.densify_split_f64(c, src, kind)
    copies = kind < 2
    assert np.array_equal(_n(out_p["xyz"])[copies], p["xyz"][copies]) and np.array_equal(_n(out_p["scaling"])[copies], p["scaling"][copies])
    rx, rsc = R.worst_ratio(_n(out_p["xyz"]), x64, xb), R.worst_ratio(_n(out_p["scaling"]), s64, sb)
    print(f"densify {name}: rows {src.size}, worst |HIP - float64| / bound: xyz {rx:.3f} scaling {rsc:.3f}")
    assert rx <= 1.0 and rsc <= 1.0


@pytest.mark.parametrize("name", ["tie scale below", "tie grad", "outcome none", "outcome all split pruned",
                                  R.width_name(R.WIDTH_CASES[5]), R.width_name(R.WIDTH_CASES[1])])
def test_densify_and_prune_on_a_model_object(dens, name):
    from splatloc_amd.densify import densify_and_prune
    from splatloc_amd.optim import Adam
    c, p, st, src, kind = dens[name]
    h = c["hyper"]
    gm = _model(c["params"], c["m"], c["v"], c["step"], Adam)
    gm.xyz_gradient_accum, gm.denom = _t(c["accum"]), _t(c["denom"])
    gm.percent_dense, gm.primitive_reg = h["percent_dense"], h["primitive_reg"]
    n = densify_and_prune(gm, h["max_grad"], h["min_opacity"], h["extent"], h["max_screen_size"], unit_noise=_t(c["unit_noise"]))
    assert n == src.size
    x64, xb, s64, sb = R.densify_split_f64(c, src, kind)
    m = {k: s["m"] for k, s in st.items()} or None
    v = {k: s["v"] for k, s in st.items()} or None
    _check_model_object(gm, p, m, v, c["step"], False, dict(xyz=(x64, xb), scaling=(s64, sb)))


@pytest.mark.parametrize("name", ["tie scale below", "tie scale at", "tie scale above"])
def test_old_plan_entry_still_plans_from_float_products(dens, name, monkeypatch):
    """splatraster_densify_plan is kept: it forms the thresholds in float32 from its float arguments.  Where that product is the
    reference's threshold, or the row on exp(0) = 1 falls on the same side of both, it plans the reference's rows; on the pair whose
    double product rounds to 1 - 2^-24 it plans the rows of the `float_products` model — the hot row cloned where the reference splits
    it: the divergence densify_tensors had before it called splatraster_densify_plan_thresholds."""
    import ctypes as C
    from splatloc_amd import _native
    from splatloc_amd.densify import densify_tensors
    c, p, st, src, kind = dens[name]
    h = c["hyper"]
    lib = _native.load()

    def old(model, acc, den, mg, mo, size_split, size_prune, usp, reg, ws, new_P, stream):
        return lib.splatraster_densify_plan(model, acc, den, mg, mo, C.c_float(h["extent"]), C.c_float(h["percent_dense"]), usp, reg,
                                            ws, new_P, stream)

    monkeypatch.setattr(lib, "splatraster_densify_plan_thresholds", old)
    out = densify_tensors({k: _t(a) for k, a in c["params"].items()}, {}, {}, _t(c["accum"]), _t(c["denom"]), h["max_grad"],
                          h["min_opacity"], h["extent"], h["max_screen_size"], h["percent_dense"], h["primitive_reg"],
                          unit_noise=_t(c["unit_noise"]), return_sources=True)
    wsrc, wkind = R.densify_plan_model(c, "float_products")
    assert np.array_equal(_n(out[3]), wsrc) and np.array_equal(_n(out[4]), wkind)
    assert (np.array_equal(wsrc, src) and np.array_equal(wkind, kind)) == (name != "tie scale below")


def test_split_draws_match_philox_and_box_muller():
    """every (seed, draw_id) with a low word, a high word or both; identity rotation, unit scales, parents at the origin: the
    children's xyz are the draws themselves, rows 0 .. P - 1, both copies"""
    from splatloc_amd.densify import densify_tensors
    P = 257
    c = R.draws_case(P)
    par = {k: _t(a) for k, a in c["params"].items()}
    accum, denom = _t(c["accum"]), _t(c["denom"])
    h = c["hyper"]
    worst, seen = 0.0, set()
    rows = np.arange(P)
    for seed in R.DRAW_WORDS:
        for did in R.DRAW_WORDS:
            out, _, _, srow, skind = densify_tensors(par, {}, {}, accum, denom, h["max_grad"], h["min_opacity"], h["extent"],
                                                     h["max_screen_size"], h["percent_dense"], h["primitive_reg"], seed=seed,
                                                     draw_id=did, return_sources=True)
            assert np.array_equal(_n(srow), np.tile(rows, 2)) and np.array_equal(_n(skind), np.repeat([2, 3], P))
            xyz = _n(out["xyz"])
            for copy in (0, 1):
                z, b = R.normal3(seed, did, rows, copy)
                worst = max(worst, R.worst_ratio(xyz[copy * P:(copy + 1) * P], z, b))
            assert not R.exceeds(np.abs(_n(out["scaling"]) - (-R.LN_1_6)), 6 * R.U + 2 * R.U * R.LN_1_6).any()
            seen.add(xyz.tobytes())
    print(f"draws: worst |HIP - float64| / bound over {len(seen)} (seed, draw_id) pairs: {worst:.3f}")
    assert worst <= 1.0 and len(seen) == len(R.DRAW_WORDS) ** 2


# ---- key-frame append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.append_case_names())
def test_extend_from_pcd_on_every_case(name):
    from splatloc_amd.densify import extend_from_pcd
    from splatloc_amd.optim import Adam
    c = R.append_case(name)
    gm = _model(c["params"], c["m"], c["v"], c["step"], Adam)
    e = c["extra"]
    n = extend_from_pcd(gm, _t(e["xyz"]), _t(c["features"]), _t(e["scaling"]), _t(e["rotation"]), _t(e["opacity"]), _t(e["marker"]),
                        _t(e["kp_score"]))
    p, m, v = R.append_expected(c)
    assert n == c["P"] + c["N"]
    _check_model_object(gm, p, m, v, c["step"], True)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
def _adam_run(c, layout, radii=None):
    """one step() of the case on fresh tensors; (params, optimizer, max_radii tensor or None)"""
    from splatloc_amd.optim import Adam
    place = _shifted if layout == "shifted" else (lambda t: t)
    params, groups = [], []
    for grp in c["groups"]:
        p = torch.nn.Parameter(place(_t(grp["p"])))
        params.append(p)
        groups.append({"params": [p], "lr": grp["lr"], "name": grp["name"]})
    opt = Adam(groups, lr=0.0, eps=R.EPS, betas=(R.BETA1, R.BETA2))
    for p, grp in zip(params, c["groups"]):
        p.grad = None if grp["g"] is None else place(_t(grp["g"]))
        if grp["step_prev"] is not None:
            opt.state[p] = {"step": torch.tensor(grp["step_prev"]), "exp_avg": place(_t(grp["m"])), "exp_avg_sq": place(_t(grp["v"]))}
    if c["gate"] is not None:
        opt.set_key_gate(_t(c["gate"][0]), c["gate"][1], c["gate"][2])
    mx = None
    if radii is not None:
        mx = _t(radii[1])
        opt.set_radii_update(_t(radii[0]), mx)
    opt.step()
    return params, opt, mx


def _adam_check(c, params, opt):
    worst = 0.0
    for p, grp in zip(params, c["groups"]):
        ref = R.adam_f64(grp, c["gate"])
        st = opt.state.get(p, {})
        if grp["g"] is None:                      # no gradient: the parameter untouched; no state, or the carried one untouched
            assert np.array_equal(_bits(_n(p)), _bits(grp["p"])), grp["name"]
            if grp["step_prev"] is None:
                assert len(st) == 0, grp["name"]
            else:
                assert float(st["step"]) == grp["step_prev"] and np.array_equal(_bits(_n(st["exp_avg"])), _bits(grp["m"]))
                assert np.array_equal(_bits(_n(st["exp_avg_sq"])), _bits(grp["v"]))
            continue
        if ref is None:                                                                   # zero elements: nothing to compare
            continue
        assert float(st["step"]) == ref["step"]
        got = dict(p=_n(p), m=_n(st["exp_avg"]), v=_n(st["exp_avg_sq"]))
        worst = max([worst] + [R.worst_ratio(got[k], ref[k], ref["b" + k]) for k in "pmv"])
    return worst


@pytest.mark.parametrize("name", R.adam_case_names())
def test_adam_step_on_every_case(name):
    c = R.adam_case(name)
    pa, oa, _ = _adam_run(c, "aligned")
    pb, ob, _ = _adam_run(c, "shifted")
    worst = _adam_check(c, pa, oa)
    for a, b in zip(pa, pb):          # the 16-byte and the scalar kernel: bit for bit the same
        assert np.array_equal(_bits(_n(a)), _bits(_n(b)))
        for k in ("exp_avg", "exp_avg_sq"):
            if k in oa.state.get(a, {}):
                assert np.array_equal(_bits(_n(oa.state[a][k])), _bits(_n(ob.state[b][k])))
    if c["gate"] is not None:         # a closed gate zeroes the gradient, it does not skip the row: an open twin differs exactly there
        open_case = dict(c, gate=None)
        po, oo, _ = _adam_run(open_case, "aligned")
        i = [g["name"] for g in c["groups"]].index(c["gate"][2])
        with np.errstate(invalid="ignore"):
            closed = c["gate"][0][:, 0] > F32(c["gate"][1])
        same = (_n(po[i]) == _n(pa[i])).reshape(closed.size, -1).all(axis=1)
        assert same[~closed].all() and (closed.sum() == 0 or not same[closed].all())
    print(f"adam {name}: worst |HIP - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_adam_step_with_the_radii_line_on_a_small_model():
    c = R.adam_case("model P5")
    radii, mx0 = np.array([3, 0, -2, 40, 1], np.int32), np.array([5.5, 1, 2, 7, np.inf], F32)
    for layout in ("aligned", "shifted"):
        pa, oa, mx = _adam_run(c, layout, (radii, mx0))
        pb, ob, _ = _adam_run(c, layout)
        assert np.array_equal(_n(mx), R.radii_expected(radii, mx0))
        assert all(np.array_equal(_bits(_n(a)), _bits(_n(b))) for a, b in zip(pa, pb))
        assert _adam_check(c, pa, oa) <= 1.0


@pytest.mark.parametrize("kind", ["quads", "elements"])
def test_adam_second_grid_pass(kind):
    """more quads (elements) than the 4096 x 256 threads of the first pass, the radii tail behind them: EVERY element against float64"""
    c = R.adam_stride_case(kind)
    n = c["groups"][0]["p"].size
    assert (n // 4 if kind == "quads" else n) > R.ADAM_QUAD_CAP
    params, opt, mx = _adam_run(c, "aligned" if kind == "quads" else "shifted", (c["radii"], c["max_radii"]))
    assert (params[0].data_ptr() % 16 == 0) == (kind == "quads")
    worst = _adam_check(c, params, opt)
    assert np.array_equal(_n(mx), R.radii_expected(c["radii"], c["max_radii"]))
    print(f"adam stride {kind}: {n} elements, worst |HIP - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- window statistics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,P,only_max", R.STATS_CASES)
def test_densification_stats_window_on_every_case(V, P, only_max):
    from splatloc_amd.densify import add_densification_stats, add_densification_stats_window
    c = R.stats_case(V, P, only_max)
    a64, ab, n_want, mx_want = R.stats_f64(c)
    runs = [lambda g, r, a, n, m: add_densification_stats_window(g, r, a, n, m)]
    if not only_max:        # the single-view entry, view after view: the same statistics
        runs.append(lambda g, r, a, n, m: [add_densification_stats(gv, rv, a, n, m) for gv, rv in zip(g, r)])
    worst = 0.0
    for run in runs:
        a, n, m = _t(c["accum"]), _t(c["denom"]), _t(c["max_radii"])
        grads, radii = [_t(c["grads"][v]) for v in range(V)], [_t(c["radii"][v]) for v in range(V)]
        if only_max:
            run(None, radii, None, None, m)
        else:
            run(grads, radii, a, n, m)
        seen = c["sees"].any(axis=0)
        assert np.array_equal(_bits(_n(m)), _bits(mx_want))                       # unseen rows keep their bits: NaN, -0.0, inf
        if only_max:
            assert np.array_equal(_bits(_n(a)), _bits(c["accum"])) and np.array_equal(_bits(_n(n)), _bits(c["denom"]))
            continue
        assert np.array_equal(_bits(_n(n)), _bits(n_want))
        assert np.array_equal(_bits(_n(a))[~seen], _bits(c["accum"])[~seen])
        worst = max(worst, R.worst_ratio(_n(a)[seen], a64[seen], ab[seen]))
    print(f"stats V{V} P{P} only_max={only_max}: worst |HIP - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- isotropic regulariser --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("SC,P,empty", [(SC, P, False) for SC, P in R.ISO_CASES] + [(3, 16385, True), (1, 5, True)])
def test_isotropic_loss_on_every_case(SC, P, empty):
    from splatloc_amd.losses import isotropic_loss
    c = R.iso_case(SC, P, empty)
    loss64, lb, grad64, gb, ok = R.iso_f64(c)
    assert ok
    s = _t(c["scaling"]).requires_grad_(True)
    loss = isotropic_loss(s, _t(c["marker"]))
    loss.backward()
    got_l, got_g = float(loss.detach()), _n(s.grad)
    assert got_g.shape == grad64.shape
    if empty or P == 0 or not (c["marker"] > R.MARKER_THR).any():
        assert got_l == 0.0 and not got_g.any() and loss64 == 0.0
        return
    assert np.array_equal(got_g == 0, grad64 == 0)                                # the mask, markers at 0.005f and around it included
    rl, rg = R.worst_ratio(got_l, loss64, lb), R.worst_ratio(got_g, grad64, gb)
    print(f"isotropic SC{SC} P{P}: worst |HIP - float64| / bound: loss {rl:.3f} gradient {rg:.3f}")
    assert rl <= 1.0 and rg <= 1.0
