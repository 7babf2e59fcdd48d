"""Host side of the decoder edge tests (tests/test_gpu_decoder_edges.py): the layouts and batch sizes are accepted and give the tile
and workgroup counts the device tests rely on, every pool yields its decided batch, and the float32 tiled model of the backward
(tests/decoder_reference.py) shows that the device tests' checks are reachable by a correct f32 implementation and fail for every
deliberately wrong one.  No GPU needed.

Measured with the f32 model, worst |model - float64| / bar: weights 0.10 (deep, N = 1), 0.032 (office_0, N = 1) and 0.017 (five160, N = 1; deep,
N = 33), below 0.012 elsewhere; table levels at most 0.0018; |loss - float64| at most 6.4e-8 (bar 1e-5)."""
import functools

import pytest
import torch

from tests import decoder_reference as R

FORWARD_NS = (1, 33, 4096, 28671, 32767, 32768, 32801)
TILES = {1: (1, 1), 33: (2, 2), 2048: (64, 64), 2049: (65, 64), 2081: (66, 64), 8225: (258, 64)}      # N: (tiles, slabs)


@functools.lru_cache(maxsize=None)
def _model(name):
    dec = R.layout_decoder(name)
    return dec, R.RestatedDecoder(dec)


@functools.lru_cache(maxsize=None)
def _batch(name, n):
    return R.edge_batch(name, _model(name)[1], n)


def _cpu(res):
    loss, gw, gt, terms = res
    return loss, [g.cpu() for g in gw], gt.cpu(), [t.cpu() for t in terms]


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(points, targets) of a named case: an int N, 'eps', 'eps_x4' (every row times 4), 'eps_x4_above' (every row above the eps
    of the cosine times 4) or 'box'"""
    if kind in ("eps", "eps_x4", "eps_x4_above"):
        pts, tgt = _batch(name, R.EPS_N)
        return pts, R.eps_targets(tgt) * R.eps_scale(kind)
    if kind == "box":
        pts, tgt = _batch(name, R.BOX_N)
        return R.box_batch(_model(name)[1], pts), tgt
    return _batch(name, kind)


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    return _cpu(R.float64_gradients(_model(name)[1], *_case(name, kind)))


@functools.lru_cache(maxsize=None)
def _got(name, kind, wrong=None):
    pts, tgt = _case(name, kind)
    return R.tiled_backward32(_model(name)[0], pts, targets=tgt, wrong=wrong)


def _align(n, a=256):
    return -(-n // a) * a


def test_office_0_of_the_builder_is_the_package_s_own_layout():
    from splatloc_amd.decoder import FeatureDecoder
    own = FeatureDecoder(R.office_0_config()).layout
    mine = _model("office_0")[0].layout
    assert mine.dims == own.dims and mine.grid.n_params == own.grid.n_params == 5_724_048
    assert mine.grid.scales == own.grid.scales and mine.grid.sizes == own.grid.sizes and (mine.bound == own.bound).all()
    for name in R.NEW_LAYOUTS:
        dec = _model(name)[0]
        spec = R.LAYOUTS[name]
        assert dec.layout.dims == spec["dims"] == [dec.layout.grid.n_output_dims] + spec["dims"][1:]
        assert [tuple(w.shape) for w in dec.feature_net.weights()] == dec.layout.weight_shapes
        assert float(dec.encoding.params.detach().abs().max()) > 0.99           # the table of uniform(-1, 1) entries
    assert [R.LAYOUTS[n]["grid"]["n_levels"] for n in R.NEW_LAYOUTS] == [8, 12, 4, 16]
    assert [R.LAYOUTS[n]["grid"]["n_features_per_level"] for n in R.NEW_LAYOUTS] == [2, 4, 8, 4]


def test_every_layout_and_batch_size_is_accepted_and_sized():
    """the workspace is [slabs: G x n_weights floats][one loss term per tile][dL/d(encoded): N x E floats], each part rounded up to
    256 bytes, so its size pins the tile and slab counts: 2048 points fill 64 slabs, 2049 open no 65th, 8225 give 258 loss terms"""
    ns = sorted(set(FORWARD_NS) | set(TILES) | set(R.TRAINER_NS))
    for name in R.LAYOUTS:
        lay = _model(name)[0].layout
        dims = lay.dims
        for n in ns:
            ws, act = lay.workspace_bytes(n)             # raises if the C entry refuses the shape
            assert act == 4 * n * (sum(dims) + 1 + 3)
            tiles, slabs = TILES.get(n, (-(-n // 32), min(-(-n // 32), 64)))
            assert ws == _align(slabs * lay.n_weights * 4) + _align(tiles * 4) + _align(n * dims[0] * 4), (name, n)
    assert set(TILES) == set(R.GRADIENT_NS) | {R.LONG_N} and R.ISOLATION_N in TILES
    assert _align(258 * 4) != _align(256 * 4)            # a 257th and 258th loss term do change the size


def test_every_pool_yields_its_batch():
    """Every (layout, N) of the gradient tests gets its N decided points from a pool of max(320, 1.1 N); the batch itself holds no
    undecided point (share 0, cap 1 %).  No output row of any batch is zero under float64.  The four replaced points of the box
    batches (both corners, a point outside, a point on a face) are decided."""
    for name, n in R.gradient_cases():
        ref = _model(name)[1]
        pts, tgt = _batch(name, n)
        assert pts.shape == (n, 3) and tgt.shape == (n, R.LAYOUTS[name]["dims"][-1])
        assert bool(ref.decided(pts).all())
        with torch.no_grad():
            out = ref(pts)
        assert bool(torch.isfinite(out).all()) and float((out.norm(dim=1) - 1).abs().max()) < 1e-12
    for name in R.LAYOUTS:
        ref = _model(name)[1]
        pool = R.points_in_bound(2400, 1)
        share = 1.0 - float(ref.decided(pool).double().mean())
        print(f"{name}: {100 * share:.2f} % of a pool of 2400 undecided")
        assert share < 0.05                                # a pool of 1.1 N is enough with room to spare
    lo, hi = torch.tensor(R.OFFICE_0, dtype=torch.float64).unbind(1)
    for name in R.BOX_LAYOUTS:
        ref = _model(name)[1]
        pts, _ = _case(name, "box")
        base, _ = _batch(name, R.BOX_N)
        assert bool(ref.decided(pts).all())
        a, b, c, d = (pts[r] for r in R.BOX_ROWS)
        assert torch.equal(a, lo) and torch.equal(b, hi)
        assert bool((((c - hi) == 0.5) | ((lo - c) == 0.5)).all())
        assert float(d[0]) == float(lo[0]) and bool((d[1:] > lo[1:]).all() and (d[1:] < hi[1:]).all())
        keep = torch.ones((R.BOX_N,), dtype=torch.bool)
        keep[list(R.BOX_ROWS)] = False
        assert torch.equal(pts[keep], base[keep])
    for name in R.EPS_LAYOUTS:
        t = _case(name, "eps")[1]
        norms = [float(t[R.EPS_ROWS[k]].double().norm()) for k in ("zero", "tiny", "seven", "milli")]
        assert norms[0] == 0.0 and 0 < norms[1] < 1e-8 and abs(norms[2] - 7) < 1e-5 and abs(norms[3] - 1e-3) < 1e-9


def _isolation_failures(name, wrong=None):
    """test 3's construction on the model: rows whose one-hot batch does not reproduce the one-point batch bit for bit"""
    dec, _ = _model(name)
    pts, _ = _batch(name, R.ISOLATION_N)
    O = dec.layout.dims[-1]
    bad = []
    for r in R.ISOLATION_ROWS:
        G = torch.zeros((R.ISOLATION_N, O))
        G[r] = R.unit_targets(1, O, 900 + r)[0]
        _, gw, gt = R.tiled_backward32(dec, pts, dL_dout=G, wrong=wrong)
        _, gw1, gt1 = R.tiled_backward32(dec, pts[r:r + 1], dL_dout=G[r:r + 1], wrong=wrong)
        same = all(torch.equal(a, b) for a, b in zip(gw, gw1)) and torch.equal(gt != 0, gt1 != 0)
        ratios = [R.row_bar_ratio(a[None], b[None]) for a, b in zip(R.level_rows(dec.layout.grid, gt), R.level_rows(dec.layout.grid, gt1))]
        if not same or max(ratios) > 1.0 or not bool(any((g != 0).any() for g in gw1)):
            bad.append(r)
    return bad


@pytest.mark.parametrize("name", ["narrow", "three"])
def test_isolation_holds_for_the_model(name):
    """a one-hot upstream gradient gives, bit for bit, the weight gradients of the one-point batch: zero rows add exact zeros to
    every chain, every slab and the slab sum"""
    assert _isolation_failures(name) == []
    assert _normalisation_holds(name) and _normalisation_holds("five160") and _normalisation_holds("office_0")


def _worst(name, kind, wrong=None):
    """(worst gradient ratio, |loss - float64|) of the model on a case"""
    want_loss, want_w, want_t, terms = _want(name, kind)
    loss, gw, gt = _got(name, kind, wrong)
    ratios = R.gradient_ratios(_model(name)[0].layout.grid, gw, gt, want_w, want_t, terms)
    return ratios, abs(float(loss) - want_loss)


def _all_cases():
    return ([(n, k) for n, k in R.gradient_cases()] + [(n, k) for n in R.EPS_LAYOUTS for k in ("eps", "eps_x4", "eps_x4_above")]
            + [(n, "box") for n in R.BOX_LAYOUTS])


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_the_model_meets_the_bars_on_every_case(layout):
    """the bars of the device tests (the project's gradient bar per weight row and table level, the loss within 1e-5) are reachable
    by a correct f32 implementation: the model meets them on every (layout, N), on the eps targets, their fourfold and the box
    batches, and its table gradient is zero exactly where the float64 one is"""
    for name, kind in [c for c in _all_cases() if c[0] == layout]:
        ratios, dloss = _worst(name, kind)
        w = max(v for k, v in ratios.items() if k.startswith("dW"))
        t = max(v for k, v in ratios.items() if k.startswith("dtable"))
        print(f"{name} {kind}: weights {w:.3g}, table {t:.3g}, |loss - float64| {dloss:.3g}")
        assert w <= 1.0 and t <= 1.0 and dloss <= 1e-5, (name, kind, ratios, dloss)
        assert torch.equal(_got(name, kind)[2] != 0, _want(name, kind)[2] != 0)
    for name in [n for n in R.EPS_LAYOUTS if n == layout]:       # scaling the targets above eps by a power of two
        (_, gw, gt), (_, gw4, gt4) = _got(name, "eps"), _got(name, "eps_x4_above")
        grid = _model(name)[0].layout.grid
        terms = _want(name, "eps")[3]
        assert max(R.gradient_ratios(grid, gw4, gt4, [g.double() for g in gw], gt.double(), terms).values()) <= 1.0
        # the zero-target row contributes nothing: the batch without it, at the same 1 / N
        pts, tgt = _case(name, "eps")
        keep = torch.arange(R.EPS_N) != R.EPS_ROWS["zero"]
        _, gwk, gtk = R.tiled_backward32(_model(name)[0], pts[keep], targets=tgt[keep], inv_n=1.0 / R.EPS_N)
        assert max(R.gradient_ratios(grid, gw, gt, [g.double() for g in gwk], gtk.double(), terms).values()) <= 1.0


def _normalisation_holds(name, wrong=None):
    """the unit-normalisation bound of the device's forward test on the model's own f: |f / norm - f / |f|| <= (gamma_O / 2 + 3 u)
    |f| / |f|.  The cosine loss and its gradient do not depend on the stored norm at all (the cosine's gradient is tangent to y,
    so the projection and the two divisions by the norm cancel any factor), which is why this defect needs the forward's check."""
    dec, _ = _model(name)
    fw = R.tiled_forward32(dec, _batch(name, 33)[0], wrong)
    f = fw["f"].double()
    want = f / f.norm(dim=-1, keepdim=True)
    got = (fw["f"] / fw["norm"][:, None]).double()
    return bool(((got - want).abs() <= (R.gamma(f.shape[1]) / 2 + 3 * R.U) * want.abs()).all())


# the cheapest cases at which each check can see each defect
EXPOSING = [("narrow", 2081), ("narrow", R.LONG_N), ("five160", 33), ("five160", "eps")]


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_wrong_model_is_exposed(wrong):
    """every deliberate defect fails at least one of the checks the device tests make: isolation, the forward's normalisation bound, the
    float64 bar, the loss"""
    failed = []
    if _isolation_failures("narrow", wrong):
        failed.append("isolation")
    if not _normalisation_holds("five160", wrong):
        failed.append("normalisation bound five160")
    for name, kind in EXPOSING:
        ratios, dloss = _worst(name, kind, wrong)
        if max(ratios.values()) > 1.0:
            failed.append(f"float64 bar {name} {kind}")
        if not dloss <= 1e-5:
            failed.append(f"loss {name} {kind}")
    print(f"{wrong}: {failed}")
    assert failed, wrong
