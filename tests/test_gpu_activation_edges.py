"""The activation stage on the device at its quad, clamp and eps edges: every case of tests/activation_reference.py through
fused.activate_pack forward and backward (activate_fwd_kernel / activate_bwd_kernel of csrc/activations.hip), the C entry points into
sentinel-filled buffers, row independence, the wrapper's input paths, the raw-parameter window path that inlines
csrc/activation_math.h, and add_densification_stats_window.  Elementwise bars of gamma(n) * sum|terms| against a float64 torch
restatement, the exact family bit for bit; tests/test_host_activation_edges.py shows on the CPU that every case reaches its edge and
that every wrong model fails.  Needs an MI355X.

Measured on an MI355X, worst |HIP - float64| / bar per quantity over the 25 cases (the case it occurred in); each test prints its own:

    scales      0.301  (cw4_p256_deg3)        d_scaling   0.299  (cw4_p257_deg0)
    rotations   0.173  (cw4_p257_deg0)        d_rotation  0.110  (cw4_p257_deg0)
    opacities   0.215  (cw3_p255_deg0)        d_opacity   0.127  (cw3_p257_deg1)
    colours     0.232  (cw5_p205_deg0)        d_f_dc      0.925  (cw3_p257_deg1; the bar is two roundings, the constant's and the product's)
    d_xyz       0.038  (cw4_p255_deg1of3)     d_f_rest    0.161  (cw4_p255_deg1of3)

the exact family (extras, d_extra, degree-0 colours and d_f_dc, isotropic scale columns, the statistics) equal bit for bit, the clamp
decided as the reference decides it on every row away from the clamp, and the three decisions consistent on every row.  No row is
skipped: the 42 rows (of 3 283; at most 10 of a case's 255, 3.9 %) whose float64 `raw` lies within the forward bar of 0 are held
to the reference evaluated with the device's own set of passing channels.

Two things missed when these tests were first run, both fixed in the kernels:
  * below the eps of normalize (||q|| < 1e-12) d_rotation kept the projection term: 5.8e6 bars off on `saturation_deg0` (row
    (3e-14, 4e-14, 0, 0), g = (1, 2, 3, 4): (0.9967, 1.9956, 3, 4)e12 for torch's (1, 2, 3, 4)e12), and the raw-parameter window with
    it.  `act_normalize_bwd` now drops the term there.
  * an isotropic log-scale past the float32 overflow of expf gave d_scaling = g0 inf + g1 inf + g2 inf, a NaN when the signs differ,
    where torch (the backward of `repeat` sums first) gives (g0 + g1 + g2) inf.  The kernel sums first now: one expf, not three.
"""
import numpy as np
import pytest
import torch

from tests import activation_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FA5A5A5          # a NaN with a payload no kernel produces
GUARD = 64
INDEPENDENCE_CASES = ("cw4_p256_deg3", "cw5_p205_deg0", "cw3_p257_deg1", "cw8_p128_deg2of3")
ENTRY_CASES = ("cw3_p255_deg0", "cw3_p257_deg1", "cw5_p204_deg2", "cw4_p255_deg1of3", "cw35_p30_deg0", "p2_cw5_deg2", "cw8_p128_deg0of3")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)       # (a copy: the cases' arrays are read-only)


def _pack(c, leaves):
    """activate_pack forward and backward on prepared leaves {name: (argument, where its gradient lands)} -> outputs by name"""
    from splatloc_amd.fused import activate_pack
    arg = {k: (None if v is None else v[0]) for k, v in leaves.items()}
    outs = activate_pack(arg["xyz"], arg["f_dc"], arg["f_rest"], arg["scaling"], arg["rotation"], arg["opacity"], extra=arg["extra"],
                         campos=_t(c["campos"]) if c["deg"] > 0 else None, active_sh_degree=c["deg"])
    loss = sum((o * _t(c["G_" + k])).sum() for o, k in zip(outs, R.FORWARD))
    loss.backward()
    torch.cuda.synchronize()
    out = {k: _np(o) for o, k in zip(outs, R.FORWARD)}
    for k in R.INPUTS:
        g = None if leaves[k] is None else leaves[k][1]()
        out["d_" + k] = None if g is None or g.numel() == 0 else _np(g.float())
    return out


def _run(c, f_rest_none=False):
    leaves = {}
    for k in R.INPUTS:
        if c[k] is None or (k == "f_rest" and f_rest_none):
            leaves[k] = None
            continue
        t = _t(c[k]).requires_grad_(True)
        leaves[k] = (t, lambda t=t: t.grad)
    return _pack(c, leaves)


@pytest.fixture(scope="module")
def measured():
    """worst |HIP - float64| / bar per quantity over the cases, printed when the module is done"""
    table = {}
    yield table
    print("\nMEASURED worst |HIP - float64| / bar per quantity (case)")
    for k, (ratio, name) in sorted(table.items()):
        print(f"    {k:12s} {ratio:6.3f}   ({name})")


def _record(measured, ratios, name):
    for k, v in ratios.items():
        print(f"RATIO {name} | {k} | {v:.3f}")
        if not (v <= measured.get(k, (-1.0, ""))[0]):
            measured[k] = (v, name)


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_within_its_bars_exact_family_and_clamp_consistency(name, measured):
    got = {}

    def run(c):
        got.update(_run(c))
        return got

    ratios = R.check_bounded(run, name)
    _record(measured, ratios, name)
    print(f"NEAR {name}: {R.near_rows(name)} of {R.case(name)['P']} rows")
    assert R.within(ratios), (name, {k: v for k, v in ratios.items() if not v <= 1.0})
    assert R.check_exact(got, name) == [], name
    assert R.check_consistency(got, name) == [], name


def _sentinel(n):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _written(buf, n):
    bits = buf.view(torch.int32)
    return bool((bits[:n] != SENTINEL).all()), bool((bits[n:] == SENTINEL).all())


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_c_entry_points_write_every_element_and_nothing_past_the_end(name):
    from splatloc_amd import _native
    from splatloc_amd._host import _ptr, _stream
    lib = _native.load()
    c = R.case(name)
    P, K, deg, SC, E = c["P"], c["K"], c["deg"], c["SC"], c["E"]
    dev = torch.device(DEV)
    t = {k: _t(c[k]) for k in R.INPUTS}
    fr = t["f_rest"] if K > 1 else None
    campos = _t(c["campos"])
    G = {k: _t(c["G_" + k]) for k in R.FORWARD}
    sizes = {"scales": 3 * P, "rotations": 4 * P, "opacities": P, "colors": (3 + E) * P}
    fwd = {k: _sentinel(n) for k, n in sizes.items()}
    head = (P, K, deg, SC, E, _ptr(t["xyz"]), _ptr(t["f_dc"]), _ptr(fr), _ptr(t["scaling"]), _ptr(t["rotation"]), _ptr(t["opacity"]))
    if deg > 0:      # refused before any launch
        assert lib.splatraster_activate_forward(*head, _ptr(t["extra"]), None, *[_ptr(fwd[k]) for k in R.FORWARD], _stream(dev)) == 1
        torch.cuda.synchronize()
        assert all(not (b.view(torch.int32) != SENTINEL).any() for b in fwd.values())
    assert lib.splatraster_activate_forward(*head, _ptr(t["extra"]), _ptr(campos), *[_ptr(fwd[k]) for k in R.FORWARD], _stream(dev)) == 0
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert _written(fwd[k], n) == (True, True), (name, k)
    ref = _run(c)
    for k, n in sizes.items():
        assert R.same_bits(_np(fwd[k][:n]).reshape(ref[k].shape), ref[k], nan_payload=True), (name, k)
    bsizes = {"d_xyz": 3 * P, "d_f_dc": 3 * P, "d_f_rest": 3 * (K - 1) * P, "d_scaling": SC * P, "d_rotation": 4 * P, "d_opacity": P,
              "d_extra": E * P}
    for with_xyz in (True, False):
        bwd = {k: _sentinel(n) for k, n in bsizes.items()}
        args = head + (_ptr(campos), *[_ptr(G[k]) for k in R.FORWARD], _ptr(bwd["d_xyz"]) if with_xyz else None, _ptr(bwd["d_f_dc"]),
                       _ptr(bwd["d_f_rest"]) if K > 1 else None, _ptr(bwd["d_scaling"]), _ptr(bwd["d_rotation"]), _ptr(bwd["d_opacity"]),
                       _ptr(bwd["d_extra"]) if E else None, _stream(dev))
        if deg > 0 and with_xyz:
            bad = list(args)
            bad[11] = None
            assert lib.splatraster_activate_backward(*bad) == 1
        assert lib.splatraster_activate_backward(*args) == 0, (name, with_xyz)      # dL_dxyz == NULL is accepted
        torch.cuda.synchronize()
        for k, n in bsizes.items():
            unwritten = (k == "d_xyz" and not with_xyz) or (k == "d_f_rest" and K == 1) or (k == "d_extra" and not E)
            assert _written(bwd[k], n) == ((not unwritten) or n == 0, True), (name, k, with_xyz)   # zeros beyond the active degree included
            if unwritten or n == 0:
                continue
            want = ref[k] if not (k == "d_xyz" and deg == 0) else np.zeros((P, 3), np.float32)
            assert R.same_bits(_np(bwd[k][:n]).reshape(want.shape), want, nan_payload=True), (name, k, with_xyz)
        if K > 1:
            M = (deg + 1) ** 2
            assert not _np(bwd["d_f_rest"][:bsizes["d_f_rest"]]).reshape(P, K - 1, 3)[:, M - 1:].any(), name


def _poisoned(c, kind_of_row):
    """a copy of case `c` whose rows i with kind_of_row(i) = 0 / 1 / 2 are NaN / infinite / a Gaussian at the camera centre; -1: kept"""
    d = dict(c)
    kinds = np.array([kind_of_row(i) for i in range(c["P"])])
    for k in R.INPUTS:
        if c[k] is None:
            continue
        a = c[k].copy()
        a[kinds == 0] = np.nan
        a[kinds == 1] = np.inf if k != "opacity" else -np.inf
        if k == "xyz":
            a[kinds == 2] = c["campos"]
        d[k] = a
    return d, kinds


@pytest.mark.parametrize("name", INDEPENDENCE_CASES)
def test_rows_are_independent_and_permute(name):
    c = R.case(name)
    P = c["P"]
    base = _run(c)
    bad, kinds = _poisoned(c, lambda i: (i // 2) % 3 if i % 2 else -1)
    assert (kinds == 0).any() and (kinds == 1).any() and (kinds == 2).any()
    got = _run(bad)
    keep = kinds == -1
    for k, a in base.items():
        if a is not None:
            assert R.same_bits(got[k][keep], a[keep], nan_payload=True), (name, k, "next to NaN, infinite and centre rows")
    perm = np.random.default_rng(3).permutation(P)
    moved = dict(c)
    for k in list(R.INPUTS) + ["G_" + q for q in R.FORWARD]:
        if c[k] is not None:
            moved[k] = np.ascontiguousarray(c[k][perm])
    got = _run(moved)
    for k, a in base.items():
        if a is not None:
            assert R.same_bits(got[k], a[perm], nan_payload=True), (name, k, "permuted")


def test_wrapper_paths():
    """f_rest as None and as [P, 0, 3]; non-contiguous and float64 inputs (what `_prep` makes of them computes the same values, bit
    for bit, as the plain float32 tensors, which test_every_case... holds to the reference); extra=None; P = 0"""
    from splatloc_amd.fused import activate_pack
    c = R.case("cw3_p255_deg0")
    assert c["K"] == 1 and c["f_rest"].shape == (255, 0, 3) and c["extra"] is None
    a, b = _run(c), _run(c, f_rest_none=True)
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or R.same_bits(a[k], b[k])), k
    for name in ("cw4_p256_deg3", "cw5_p205_deg0"):
        c = R.case(name)
        plain = _run(c)
        strided, doubles = {}, {}
        for k in R.INPUTS:
            v = _t(c[k])
            big = torch.zeros(v.shape[:-1] + (2 * v.shape[-1],), device=DEV)
            big[..., ::2] = v
            big.requires_grad_(True)
            view = big[..., ::2]
            assert v.numel() == 0 or v.shape[-1] == 1 or not view.is_contiguous()
            strided[k] = (view, lambda big=big: None if big.grad is None else big.grad[..., ::2])
            d = v.double().requires_grad_(True)
            doubles[k] = (d, lambda d=d: d.grad)
        for what, leaves in (("non-contiguous", strided), ("float64", doubles)):
            got = _pack(c, leaves)
            for k, a in plain.items():
                assert (a is None) == (got[k] is None) and (a is None or R.same_bits(got[k], a)), (name, what, k)
    z = lambda *s: torch.zeros(s, device=DEV, requires_grad=True)  # noqa: E731
    leaves = (z(0, 3), z(0, 1, 3), z(0, 3, 3), z(0, 3), z(0, 4), z(0, 1))
    outs = activate_pack(*leaves, extra=None, campos=torch.zeros(3, device=DEV), active_sh_degree=1)
    assert [tuple(o.shape) for o in outs] == [(0, 3), (0, 4), (0, 1), (0, 3)]
    sum(o.sum() for o in outs).backward()
    torch.cuda.synchronize()
    assert all(t.grad is None or t.grad.numel() == 0 for t in leaves)


def test_raw_parameter_window_is_activate_plus_window_bit_for_bit():
    """The edge rows that keep the rasterizer finite (saturated logits, the clamp triple, scaled, zero and sub-eps quaternions) as 49
    visible Gaussians of a 64 x 64 frame: window_forward(raw=) / window_backward(raw=) against activate_forward + window +
    activate_backward, the contract csrc/activation_math.h states, with the deterministic-sum compositing."""
    from splatloc_amd import _native, rasterizer
    from splatloc_amd.camera import PinholeCamera
    from splatloc_amd.fused import _view_settings, activate_backward, activate_forward
    import types
    rows = R.raw_path_rows()
    P = rows["opacity"].shape[0]
    assert P == 49 and np.isfinite(rows["scaling"]).all() and np.isfinite(rows["rotation"]).all()
    W = H = 64
    gy, gx = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
    xyz = np.stack([(gx.ravel() - 3) * 0.45, (gy.ravel() - 3) * 0.45, np.full(P, 2.0)], 1).astype(np.float32)
    cam = PinholeCamera(W, H, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, torch.eye(3), torch.zeros(3)).to(DEV)
    pc = types.SimpleNamespace(active_sh_degree=0)
    settings = [_view_settings(cam, pc, torch.zeros(3, device=DEV), 1.0)]
    t = {k: _t(v) for k, v in rows.items()}
    m3 = _t(xyz)
    g = torch.Generator().manual_seed(9)
    grads = [(torch.randn(3, H, W, generator=g).to(DEV), torch.randn(H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV), None)]
    raw = (t["scaling"], t["rotation"], t["opacity"], t["f_dc"], t["extra"])
    _native.set_deterministic(True)
    try:
        fr = rasterizer.window_forward(m3, None, None, None, None, None, settings, raw=raw)
        dr = rasterizer.window_backward(fr, grads, 3, raw=raw)
        (scales, rotations, opacities, colors), act = activate_forward(m3, t["f_dc"], None, t["scaling"], t["rotation"], t["opacity"],
                                                                       t["extra"], None, 0)
        fp = rasterizer.window_forward(m3, colors, opacities, scales, rotations, None, settings)
        dp = rasterizer.window_backward(fp, grads, 3)
        _dx, d_fd, _fr, d_sc, d_ro, d_op, d_ex = activate_backward(act, dp["sca"], dp["rot"], dp["op"], dp["col"])
        torch.cuda.synchronize()
    finally:
        _native.set_deterministic(False)
    assert int((fr.radii > 0).sum()) == P and fr.R == fp.R                       # every edge row is visible
    bits = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731
    for k, a, b in (("scales", fr.sca, scales), ("rotations", fr.rot, rotations), ("opacities", fr.opa, opacities), ("colors", fr.col, colors),
                    ("image", fr.color, fp.color), ("depth", fr.depth, fp.depth), ("alpha", fr.alpha, fp.alpha), ("m3", dr["m3"], dp["m3"]),
                    ("scaling", dr["scaling"], d_sc), ("rotation", dr["rotation"], d_ro), ("opacity", dr["opacity"], d_op),
                    ("f_dc", dr["f_dc"], d_fd), ("extra", dr["extra"], d_ex)):
        assert torch.isfinite(a).all(), k
        assert bits(a, b), (k, float((a - b).abs().max()))
    # and the chain itself follows torch's rule below the eps: d_rotation = g / 1e-12 exactly, g being the rasterizer's dL/drotations
    sub = [10, 11, 13, 14]
    assert bits(dr["rotation"][sub], dp["rot"][sub] / torch.tensor(1e-12, device=DEV))
    assert float(dr["rotation"][sub].abs().max()) > 0


def _stats_run(grads, radii, accum, denom, maxr):
    from splatloc_amd.densify import add_densification_stats_window
    ta, td, tm = _t(accum), _t(denom), _t(maxr)
    add_densification_stats_window(None if ta is None else [_t(g) for g in grads], [_t(r) for r in radii], ta, td, tm)
    torch.cuda.synchronize()
    return _np(ta), _np(td), _np(tm)


@pytest.mark.parametrize("V", [1, 2, 8])
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_densification_stats_window_is_the_sequential_model(P, V):
    assert R.check_stats(_stats_run, P, V) == []
