"""The per-Gaussian projection on the device at its cull, clamp and tile-rect edges: every case of tests/projection_reference.py through
the forward (preprocess_kernel: per view, window, raw parameters) and through every entry point that inlines the shared backward of
csrc/projection_bwd.h — view_backward without and with pose gradients (preprocess_bwd_kernel<POSE>), window_backward plain and raw,
window_backward_cameras (camera_bwd_kernel) and window_backward(cameras=True) (window_joint_bwd_kernel).  Radii, tile counts,
num_rendered and the first record are bit-identical to the CPU oracle and the decisions exact against the float64 reference; conic and
pixel records and every gradient row lie within the case's bound of the reference (max(4 E_oracle, n 2^-24) of the row's own maximum),
rows the reference holds at exact zero are exact zeros, and so are the entries of the camera gradients that no Gaussian writes.
tests/test_host_projection_edges.py proves on the CPU that every case reaches its edge and that every wrong model exceeds these bounds.
Needs an MI355X.

Measured on an MI355X: the device's deviation over the bound, the worst output of each group over every path the case runs through
(records: pix, tz, conic; params: every parameter gradient; camera: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos; the last column: the
camera-only and the joint kernel against the per-view calls, in the same unit).  A ratio of 0.25 is the oracle's own deviation: where
it stands, the device deviates from the reference as far as the oracle does, to three digits — both by the float32 rounding of the same
forward records (a pixel centre known to 4e-6 px under a loss pixel one deviation away: tests/projection_reference.py, sensitivity).
The bounds themselves are between 2.9e-6 (the floor, 48 * 2^-24, for the camera tensors as well) and 2.9e-5 of a row's maximum, 4.5e-5 in
`long thin off-axis` (tests/projection_reference.py).

    case                     records  params  means2D   camera   camera vs per-view call
    cull                      0.133    0.128    0.056    0.025    0.000
    clamp x                   0.159    0.282    0.250    0.114    0.000
    clamp y cov3D             0.146    0.261    0.252    0.256    0.000
    clamp xy modifier 1.6     0.250    0.365    0.254    0.276    0.000
    conic and radius          0.099    0.328    0.250    0.203    0.000
    long thin off-axis        0.250    0.221    0.413    0.312    0.000
    rect 33x33                0.114    0.266    0.230    0.213    0.000
    rect ragged 40x24         0.080    0.284    0.272    0.145    0.000
    p_w epsilon               0.125    0.259    0.118    0.131    0.000
    block P 1                 0.053    0.250    0.045    0.069    0.000
    block P 255               0.084    0.250    0.245    0.255    0.017
    block P 256               0.084    0.250    0.232    0.247    0.000
    block P 257               0.084    0.255    0.245    0.277    0.000
    block P 513               0.084    0.252    0.250    0.272    0.000
    window V 2                0.250    0.323    0.250    0.243    0.000
    window V 5                0.250    0.250    0.248    0.255    0.000
    window V 8                0.250    0.276    0.250    0.268    0.000
    channels 3                0.250    0.324    0.250    0.248    0.000
    channels 4                0.250    0.270    0.250    0.111    0.000
    channels 35               0.250    0.257    0.231    0.184    0.000
    channels 40               0.250    0.265    0.244    0.139    0.006
    sh degree 2               0.250    0.260    0.250    0.293        -
    raw cull E 0              0.086    0.129    0.144        -        -
    raw clamp x E 1           0.159    0.313    0.250        -        -
    raw window V 5 E 1        0.250    0.308    0.258        -        -
    raw window V 2 E 0        0.250    0.327    0.260        -        -
    non-finite means          0.125        -        -        -        -

Two outputs missed when these tests were first run.
  * `sh degree 2`, dL/dcampos through view_backward with pose gradients: 49.0 * 2^-24 of the tensor's largest entry against a bound of
    48.4 (4 E_oracle; the floor is 48): 1.012 of it.  preprocess_bwd_kernel took the camera centre's term back OUT of dL/dmeans3D, as
    (dmean behind sh_backward) - (dmean in front of it), and so with the rounding of the projection's part of dmean, which is the
    larger one.  sh_backward now adds into a zeroed triple that is joined to dmean afterwards (the same dL/dmeans3D, bit for bit:
    0 + term is exact) and IS the camera centre's term: 0.293 of the bound.
  * `conic and radius` held a 1 : 1 : 100 Gaussian turned 30 degrees off the image axis at a footprint of 4 px by 0.55 px: dL/dscales
    of its long axis came out 9.1e-6 of the row's maximum off, 1.44 of the bound (6.4e-6), through view_backward.  A float32 numpy
    transcription of the formulas of projection_row_bwd + sigma3_chain_bwd, fed with the oracle's float64 moments, is off by 6.6e-6
    (median) to 2.8e-5 on that row over 300 inputs a few ulps apart: det = a c - b b returned the roundings of a, b, c
    (a c + b b) / det = 11-fold there, against at most 2.2-fold in every other case.  The floor counts every rounding once, so the
    builders assert that factor to be at most 4 (projection_reference.ill_conditioned) and the Gaussian of that case kept its
    1 : 1 : 100 and its 30 degrees at a footprint of 1.5 px (factor 2.3).  The 4 px footprint, its mirror at 60 degrees and one along
    the axis moved into a case of their own, `long thin off-axis`, whose floor on the gradients chained through dL/dcov2D is
    kappa-fold (15.7 * 48 * 2^-24 = 4.5e-5; a deviation from the issue's floor, named in tests/projection_reference.py): the kernels
    use 0.12 of it, 5.3e-6 of the row's maximum at the worst.  No kernel was changed for this one.
"""
import numpy as np
import pytest
import torch

from tests import projection_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("m3", "op", "col", "sca", "rot", "cov", "sh")
RAW_PARAMS = ("m3", "scaling", "rotation", "opacity", "f_dc", "extra")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _settings(c, v):
    from splatloc_amd import GaussianRasterizationSettings
    Vn, PMn, cpn = c.views[v]
    return GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, _t(c.bg), c.mod, _t(Vn), _t(PMn), c.sh_degree, _t(cpn), False, False)


@pytest.fixture(scope="module")
def measured():
    """worst deviation / bound per (path, output), printed when the module is done (the table of the docstring)"""
    table = {}
    yield table
    print("\nMEASURED deviation / bound, worst case per path and output")
    for (path, k), (ratio, name) in sorted(table.items()):
        print(f"    {path:24s} {k:10s} {ratio:6.3f}   ({name})")


def _within(c, E, path, k, got, ref, measured):
    dev, bnd = R.deviation(c, k, got, ref), R.bound(c, k, E[k])
    ratio = dev / bnd
    print(f"RATIO {c.name} | {path} | {k} | {ratio:.3f}")
    if not (ratio <= measured.get((path, k), (-1.0, ""))[0]):
        measured[(path, k)] = (ratio, c.name)
    if not dev <= bnd:
        rows = R.deviation(c, k, got, ref, per_row=True)
        worst = int(np.argmax(rows))
        raise AssertionError(f"{c.name}, {path}, {k}: deviation {dev:.3e} of the row maximum, bound {bnd:.3e} ({ratio:.2f} of it); per row / bound "
                             f"{np.round(rows / bnd, 2).tolist()}; row {worst}: {np.asarray(got).reshape(rows.size, -1)[worst].tolist()} for "
                             f"{np.asarray(ref).reshape(rows.size, -1)[worst].tolist()}")


def _check_forward(c, path, measured, radii, recs, tiles, num_rendered):
    """radii [V,P], recs [V,P,8], tiles [V,P], num_rendered [V] of the device against the oracle (bits) and the reference"""
    ref, orc, E = R.reference(c), R.oracle_run(c), R.oracle_errors(c)
    rec0 = np.ascontiguousarray(recs[..., :4])
    assert np.array_equal(radii, orc["radii"]) and np.array_equal(tiles, orc["tiles"]), (c.name, path)
    assert [int(r) for r in num_rendered] == [int(r) for r in orc["num_rendered"]], (c.name, path)     # no padding lane counted
    assert np.array_equal(rec0.view(np.uint32), orc["rec0"].view(np.uint32)), (c.name, path)
    got = dict(ok=radii > 0, radii=radii, tiles=tiles, num_rendered=np.asarray(num_rendered))
    assert R.decisions_differ(got, ref) == [], (c.name, path)
    culled = ~ref["ok"]
    assert not recs[culled].view(np.uint32).any(), "a culled row's records are zeros"
    _within(c, E, path, "pix", recs[..., 0:2], ref["pix"], measured)
    _within(c, E, path, "tz", recs[..., 2], ref["tz"], measured)
    _within(c, E, path, "conic", recs[..., 4:7], ref["conic"], measured)
    opa = R.plain_inputs(c)[0].reshape(-1)
    if c.raw is None:
        assert np.array_equal(recs[..., 7][ref["ok"]], np.broadcast_to(opa, ref["ok"].shape)[ref["ok"]])


def _check_grads(c, path, measured, d, names, view=None):
    """gradients `d` of the device against the reference; `view`: d belongs to that view alone (a per-view call on a window case:
    only its means2D and camera gradients are compared)"""
    ref, E = R.reference(c), R.oracle_errors(c)
    for k in names:
        if ref[k] is None:
            assert d.get(k) is None, (c.name, path, k)
            continue
        _within(c, E, path, k, _np(d[k]).reshape(ref[k].shape), ref[k], measured)
    m2 = _np(d["m2"])
    assert not m2[..., 2].any(), "the third column of dL/dmeans2D"
    _within(c, E, path, "m2", m2[..., :2].reshape(-1, c.P, 2), ref["m2"] if view is None else ref["m2"][view:view + 1], measured)
    if d.get("view") is not None:
        sel = slice(None) if view is None else slice(view, view + 1)
        gv, gp, gc = _np(d["view"]).reshape(-1, 4, 4), _np(d["proj"]).reshape(-1, 4, 4), _np(d["campos"]).reshape(-1, 3)
        zv, zp = R.structural_zeros(gv, gp)
        assert not zv.any() and not zp.any() and (c.shs is not None or not gc.any()), (c.name, path)
        _within(c, E, path, "view", gv, ref["view"][sel], measured)
        _within(c, E, path, "proj", gp, ref["proj"][sel], measured)
        _within(c, E, path, "campos", gc, ref["campos"][sel], measured)
        return gv, gp
    return None


def _plain_tensors(c):
    opa, col, sca, rot = R.plain_inputs(c)
    return dict(m3=_t(c.means3D), shs=_t(c.shs), col=_t(col) if c.shs is None else None, opa=_t(opa), sca=_t(sca) if c.cov is None else None,
                rot=_t(rot) if c.cov is None else None, cov=_t(c.cov))


def _view_state(f, P):
    from splatloc_amd import introspect
    g = introspect.geometry_views(f.geom, P)
    return (_np(f.radii)[None], np.concatenate([_np(g["rec0"]), _np(g["rec1"])], axis=1)[None], _np(g["tiles_touched"]).astype(np.int64)[None],
            [f.num_rendered])


def _window_state(c, f):
    from splatloc_amd import introspect
    st = introspect.window_state((f.geom, f.binning, f.img), c.P, c.V, c.W, c.H, f.R)
    recs = np.stack([np.concatenate([_np(s["rec0"]), _np(s["rec1"])], axis=1) for s in st])
    return _np(f.radii), recs, np.stack([_np(s["tiles_touched"]).astype(np.int64) for s in st]), f.R


@pytest.mark.parametrize("name", [n for n in R.case_names(backward=True) if not n.startswith("raw ")])
def test_per_view_calls(name, measured):
    """view_forward, then view_backward without and with pose gradients, on every view of the case by itself"""
    from splatloc_amd import rasterizer
    c = R.case(name)
    T = _plain_tensors(c)
    cams = []
    for v in range(c.V):
        f = rasterizer.view_forward(T["m3"], T["shs"], T["col"], T["opa"], T["sca"], T["rot"], T["cov"], _settings(c, v))
        torch.cuda.synchronize()
        radii, recs, tiles, nr = _view_state(f, c.P)
        if c.V == 1:
            _check_forward(c, "view_forward", measured, radii, recs, tiles, nr)
        else:
            orc = R.oracle_run(c)
            assert np.array_equal(radii[0], orc["radii"][v]) and np.array_equal(tiles[0], orc["tiles"][v]) and nr[0] == orc["num_rendered"][v]
            assert np.array_equal(np.ascontiguousarray(recs[0, :, :4]).view(np.uint32), orc["rec0"][v].view(np.uint32))
        grads = [_t(g) for g in c.grads[v]]
        only = None if c.V == 1 else v
        d0 = rasterizer.view_backward(f, *grads, want_pose=False)
        d1 = rasterizer.view_backward(f, *grads, want_pose=True)
        torch.cuda.synchronize()
        assert d0["view"] is None and d0["proj"] is None
        _check_grads(c, "view_backward", measured, d0, PARAMS if c.V == 1 else (), only)
        cams.append(_check_grads(c, "view_backward pose", measured, d1, PARAMS if c.V == 1 else (), only))
    if c.shs is None:
        _camera_paths(c, measured, cams)


def _window_grads(c):
    return [(_t(gc), None, _t(gd), _t(ga)) for gc, gd, ga in c.grads]


def _camera_paths(c, measured, per_view):
    """window_forward, window_backward, window_backward_cameras and the joint call on the case's window (V = 1: a window of one view);
    the camera-only and the joint kernel against the per-view calls `per_view` [(dV, dPM)] within the bound as well"""
    from splatloc_amd import rasterizer
    T = _plain_tensors(c)
    f = rasterizer.window_forward(T["m3"], T["col"], T["opa"], T["sca"], T["rot"], T["cov"], [_settings(c, v) for v in range(c.V)])
    torch.cuda.synchronize()
    _check_forward(c, "window_forward", measured, *_window_state(c, f))
    d = rasterizer.window_backward(f, _window_grads(c))
    torch.cuda.synchronize()
    assert "view" not in d
    _check_grads(c, "window_backward", measured, d, PARAMS)
    dc = rasterizer.window_backward_cameras(f, [tuple(_t(g) for g in gs) for gs in c.grads])
    dj = rasterizer.window_backward(f, _window_grads(c), cameras=True)
    torch.cuda.synchronize()
    _check_grads(c, "window_backward joint", measured, dj, PARAMS)
    ref, E = R.reference(c), R.oracle_errors(c)
    pv = np.stack([p[0][0] for p in per_view]), np.stack([p[1][0] for p in per_view])
    for path, got in (("window_backward_cameras", dc), ("window_backward joint", dj)):
        gv, gp, gc = _np(got["view"]), _np(got["proj"]), _np(got["campos"])
        zv, zp = R.structural_zeros(gv, gp)
        assert not zv.any() and not zp.any() and not gc.any(), (c.name, path)
        _within(c, E, path, "view", gv, ref["view"], measured)
        _within(c, E, path, "proj", gp, ref["proj"], measured)
        _within(c, E, path + " vs per view", "view", gv, pv[0], measured)
        _within(c, E, path + " vs per view", "proj", gp, pv[1], measured)


@pytest.mark.parametrize("name", [n for n in R.case_names(backward=True) if n.startswith("raw ")])
def test_raw_parameter_window(name, measured):
    """window_forward(raw=) / window_backward(raw=): the activations inside the projection kernel and its backward, against the same
    reference composed with exp / normalize / sigmoid / degree-0 SH"""
    from splatloc_amd import rasterizer
    c = R.case(name)
    assert c.raw is not None
    raw = tuple(_t(a) for a in c.raw)
    f = rasterizer.window_forward(_t(c.means3D), None, None, None, None, None, [_settings(c, v) for v in range(c.V)], raw=raw)
    torch.cuda.synchronize()
    _check_forward(c, "window_forward raw", measured, *_window_state(c, f))
    d = rasterizer.window_backward(f, _window_grads(c), raw=raw)
    torch.cuda.synchronize()
    _check_grads(c, "window_backward raw", measured, d, RAW_PARAMS)


@pytest.mark.parametrize("name", ["cull", "raw cull E 0", "window V 5"])
def test_mark_visible_takes_the_cull_decision(name):
    from oracle import oracle
    from splatloc_amd import GaussianRasterizer
    c = R.case(name)
    ref = R.reference(c)
    for v in range(c.V):
        got = _np(GaussianRasterizer(_settings(c, v)).markVisible(_t(c.means3D)))
        assert np.array_equal(got, ref["in_front"][v]) and np.array_equal(got, oracle.mark_visible(c.means3D, c.views[v][0])), (name, v)


def test_non_finite_means_forward(measured):
    """A NaN and an infinite mean next to healthy Gaussians, forward only: they are culled, their rows are the oracle's bit for bit
    (zeros), and the healthy Gaussians' decisions and records are what they are without them.
    An infinite or NaN SCALE is not run: by reading, preprocess_kernel gives such a Gaussian the radius f2i_sat(NaN) = -1e9, the
    rectangle [gx, 0) x [gy, 0) and with it a POSITIVE area (the product of two negative extents) and gx * gy tiles; emit_kernel
    (csrc/binning.hip) then forms tile keys from the origin gy * gx + gx and the width 0 - gx, which lie outside the range table."""
    from splatloc_amd import rasterizer
    c = R.case("non-finite means")
    T = _plain_tensors(c)
    f = rasterizer.view_forward(T["m3"], None, T["col"], T["opa"], T["sca"], T["rot"], None, _settings(c, 0), forward_only=True)
    torch.cuda.synchronize()
    _check_forward(c, "view_forward", measured, *_view_state(f, c.P))
    fw = rasterizer.window_forward(T["m3"], T["col"], T["opa"], T["sca"], T["rot"], None, [_settings(c, 0)], forward_only=True)
    torch.cuda.synchronize()
    _check_forward(c, "window_forward", measured, *_window_state(c, fw))
    assert torch.isfinite(f.color).all() and torch.equal(f.color, fw.color[0])
