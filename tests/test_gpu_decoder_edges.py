"""The fused FeatureDecoder on the MI355X at its tile, slab and layout edges: every layout the C entry accepts that office_0 does not
reach (tests/decoder_reference.py LAYOUTS: E = 16 / 48 / 64, H = 32 / 64 / 128, O = 32 / 96 / 160 / 256, 2 / 3 / 5 / 8 layers, F = 2 /
4 / 8, 4 / 8 / 12 / 16 levels), both tile heights of the forward, the backward beyond one round of its 64 workgroups (N > 2048), the
strided loss reduction (N > 8192), partial last tiles, the eps branches of the cosine and points on and outside the box.
tests/test_host_decoder_edges.py shows on a float32 model that these checks fail for every deliberately wrong backward.

Measured on the MI355X, worst |device - bound or float64| / bar (each test's docstring has its own figures): forward layers 0.29;
one-hot isolation: all 21 (layout, row) pairs bit-identical, table included; gradients 0.037 and below except one entry of `deep`
at N = 1 (1.16 under the plain bar, 0.124 with its float64 conditioning term, see test_gradients_match_float64_beyond_one_round);
table levels 0.0019; losses within 6.4e-8 (bar 1e-5); trainer 0.35."""
import functools

import pytest
import torch

from tests import decoder_reference as R

pytestmark = pytest.mark.gpu

LR = 1e-3


@functools.lru_cache(maxsize=None)
def _model(name):
    """(decoder, float64 restatement) of a layout, shared by the tests and never modified"""
    dec = R.layout_decoder(name)
    return dec, R.RestatedDecoder(dec)


@functools.lru_cache(maxsize=None)
def _batch(name, n):
    return R.edge_batch(name, _model(name)[1], n)


@functools.lru_cache(maxsize=None)
def _want(name, n):
    return R.float64_gradients(_model(name)[1], *_batch(name, n))


@functools.lru_cache(maxsize=None)
def _cloud(n=32801):
    return R.points_in_bound(n, 11)


def _check(dec, gw, gt, want_w, want_t, terms, what):
    """the project's gradient bar per weight row (plus the float64 conditioning term, R.float64_gradients) and per table level;
    prints the worst ratio of every weight matrix and of the table, and the worst entry without the conditioning term"""
    ratios = R.gradient_ratios(dec.layout.grid, gw, gt, want_w, want_t, terms)
    w = {k: v for k, v in ratios.items() if k.startswith("dW")}
    t = max(v for k, v in ratios.items() if k.startswith("dtable"))
    plain = max((R.worst_entry(g, ww, tt) + (l,) for l, (g, ww, tt) in enumerate(zip(gw, want_w, terms))), key=lambda e: e[0])
    print(f"{what}: worst |got - want| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f", table {t:.3g}; "
          f"without the conditioning term {plain[0]:.3g} at dW{plain[4]}[{plain[1]}][{plain[2]}], kappa {plain[3]:.3g}")
    assert max(ratios.values()) <= 1.0, (what, ratios)


def _autograd_gradients(dec, pts, G=None, tgt=None):
    """([dW_l], dtable) through _DecoderFunction: out.backward(G), or cos_loss(out, tgt).backward(); leaves no .grad behind"""
    from splatloc_amd.decoder import cos_loss
    dec.zero_grad()
    out = dec(pts)
    if G is not None:
        out.backward(G.cuda())
    else:
        cos_loss(out, tgt.cuda()).backward()
    gw = [w.grad.clone() for w in dec.feature_net.weights()]
    gt = dec.encoding.params.grad.clone()
    dec.zero_grad()
    return gw, gt


@pytest.mark.parametrize("N", [1, 33, 32801])
@pytest.mark.parametrize("name", R.NEW_LAYOUTS)
def test_layers_within_the_fma_chain_bound_per_layout(name, N):
    """test_layers_within_the_fma_chain_bound of tests/test_gpu_decoder.py on the four layouts it does not reach, with the same
    analytic bars: every layer recomputed in float64 from the device's own input activations lies within gamma_K * |a| @ |w|^T, the
    stored norm within (gamma_O / 2 + 2 u) and the output within (gamma_O / 2 + 3 u) of the exact normalisation of the device's f.
    N = 32801 = 32768 + 33 runs the 64-point tiles, its last tile with one live row in its second 32-row block.  The inference
    launch gives the training launch's bits.
    Measured, worst |device - f64| / bar over the layers: narrow 0.033 / 0.15 / 0.29 (N = 1 / 33 / 32801), three 0.039 / 0.044 /
    0.096, five160 0.031 / 0.10 / 0.13, deep 0.018 / 0.040 / 0.086."""
    from tests.test_gpu_decoder import _training_forward
    dec, _ = _model(name)
    O = dec.layout.dims[-1]
    pts = _cloud()[:N]
    out, rec = _training_forward(dec, pts)
    assert out.shape == (N, O) and out.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(dec(pts), out)
    ws = [w.detach().double() for w in dec.feature_net.weights()]
    worst = []
    for l, w in enumerate(ws):
        a = rec["inputs"][l].double()
        pre = a @ w.t()
        bar = R.gamma(w.shape[1]) * (a.abs() @ w.abs().t())
        got = (rec["inputs"][l + 1] if l + 1 < len(ws) else rec["f"]).double()
        want = torch.relu(pre) if l + 1 < len(ws) else pre
        worst.append(float(((got - want).abs() / bar.clamp_min(1e-300)).max()))
        assert float(((got - want).abs() - bar).max()) <= 0.0, (l, worst)
    print(f"{name} N={N}: worst |device - f64| / bar per layer = " + ", ".join(f"{v:.3g}" for v in worst))
    f = rec["f"].double()
    n64 = f.norm(dim=-1, keepdim=True)
    assert bool((n64 > 0).all())
    nbar = R.gamma(O) / 2
    assert bool(((rec["norm"].double()[:, None] - n64).abs() <= (nbar + 2 * R.U) * n64).all())
    assert bool(((out.double() - f / n64).abs() <= (nbar + 3 * R.U) * (f / n64).abs()).all())


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_tile_heights_give_the_same_bits(name):
    """Localisation decodes whole maps (64-point tiles from N = 32768), training decodes batches (32-point tiles): an output row
    is the same k-ordered chain whatever the tile height and wherever the row stands in its tile.  dec(pts[:32801]) (64-point
    tiles) equals the concatenation of dec(pts[:4096]), dec(pts[4096:32767]) and dec(pts[32767:32801]) (32-point tiles, at three
    different row offsets) bit for bit, and N = 32767 and N = 32768, either side of the switch, agree on their common rows."""
    dec, _ = _model(name)
    pts = _cloud()
    with torch.no_grad():
        whole = dec(pts)
        parts = torch.cat([dec(pts[:4096]), dec(pts[4096:32767]), dec(pts[32767:])])
        below, above = dec(pts[:32767]), dec(pts[:32768])
    assert whole.shape == (32801, dec.layout.dims[-1]) and bool(torch.isfinite(whole).all())
    assert torch.equal(whole, parts)
    assert torch.equal(below, above[:32767]) and torch.equal(above, whole[:32768])


@pytest.mark.parametrize("name", R.ISOLATION_LAYOUTS)
def test_a_one_hot_upstream_gradient_isolates_a_point_exactly(name):
    """Through _DecoderFunction (the dL_dout route, which has no 1 / N): with G zero except row r of a 2081-point batch (66
    tiles), every MLP weight gradient is bit-identical to that of the one-point batch pts[r:r+1] with G[r:r+1].  Zero rows of dPre
    add exact zeros to every MFMA chain, to every slab and to the ascending slab sum, so any tile, slab or live-row indexing error
    shows with no tolerance.  Rows: first and last of tile 0, first of tile 1, last of the last first-round tile (2047), first of
    the first second-round tile (2048: workgroup 0's accumulate path), and the last full and the partial last tile (2079, 2080).
    The table gradient (an arrival-ordered atomic scatter) meets the per-level bar and has exactly the same non-zero entries.
    Measured: weights identical at every row of every layout; the table gradients were bit-identical as well (ratio 0)."""
    dec, _ = _model(name)
    pts, _ = _batch(name, R.ISOLATION_N)
    O = dec.layout.dims[-1]
    grid = dec.layout.grid
    for r in R.ISOLATION_ROWS:
        G = torch.zeros((R.ISOLATION_N, O))
        G[r] = R.unit_targets(1, O, 900 + r)[0]
        gw, gt = _autograd_gradients(dec, pts, G=G)
        gw1, gt1 = _autograd_gradients(dec, pts[r:r + 1], G=G[r:r + 1])
        assert all(bool((g != 0).any()) for g in gw1), r
        for l, (a, b) in enumerate(zip(gw, gw1)):
            assert torch.equal(a, b), (name, r, l, float((a - b).abs().max()))
        assert torch.equal(gt != 0, gt1 != 0) and int((gt1 != 0).sum()) > 0, (name, r)
        worst = max(R.row_bar_ratio(a[None], b[None]) for a, b in zip(R.level_rows(grid, gt), R.level_rows(grid, gt1)))
        print(f"{name} row {r}: weights identical, table worst |batch - single| / bar = {worst:.3g}")
        assert worst <= 1.0, (name, r, worst)


@pytest.mark.parametrize("name,N", R.gradient_cases(), ids=[f"{a}-{b}" for a, b in R.gradient_cases()])
def test_gradients_match_float64_beyond_one_round(name, N):
    """cos_loss_and_gradients against float64 autograd of the restatement on decided batches, with the bars of
    test_gradients_match_float64: 1e-4 |want| + 1e-3 of the row's maximum per weight row and per table level, the loss within 1e-5.
    N = 1 and 33: one tile and a one-row second tile; 2048: 64 tiles, every workgroup one tile; 2049 and 2081: workgroups 0 (and 1)
    add a second tile into their slab, 2081 with a partial last tile; 8225: 258 tiles, four rounds and the strided part of the loss
    reduction.  The table gradient is zero exactly where float64's is, the autograd route meets the same bars, and at N = 2081 and
    8225 the loss and the weight gradients of two identical calls are bit-identical.
    One entry needs more than the project's bar, and float64 says which.  `deep`, N = 1: dW0[48][37] misses the plain bar at 1.16
    (0.45 by the autograd route, another rounding of the same entry).  With one point a row of dW0 is dPre0[o] times the encoded
    features, so the row's maximum is that entry itself, and dPre0[48] = 1.7e-5 is a 128-term chain whose terms cancel 9160-fold
    under float64 (the row's median entry is 1.8e-2): the device's absolute error, 2e-8, is what every other entry of that chain
    carries.  So a weight entry whose terms cancel more than a thousandfold under float64 gets 1e-6 of the absolute sum of its
    terms on top (R.float64_gradients, R.row_bar_ratio; the term test_first_three_reference_steps uses for the same reason); every
    other entry is held to the plain bar.  Each line printed names the worst entry under the plain bar and its kappa.
    Measured, worst |device - float64| / plain bar over the weights (fused route; the autograd route is within 15 % of it):
    N = 1: office_0 0.037, narrow 0.0010, three 0.0047, five160 0.015, deep 1.16 (0.124 with the term);
    N = 33: 0.0016, 0.00051, 0.00075, 0.020, 0.019;  N = 2048: 0.0014, 0.00052, 0.00067, 0.0015, 0.0034;
    N = 2049: 0.00096, 0.00059, 0.00069, 0.0017, 0.0024;  N = 2081: 0.0011, 0.00046, 0.00095, 0.0010, 0.0024;
    N = 8225: office_0 0.00093, narrow 0.00064.  Table levels: at most 0.0019.  |loss - float64| at most 6.4e-8."""
    from splatloc_amd.decoder import cos_loss_and_gradients
    dec, _ = _model(name)
    pts, tgt = _batch(name, N)
    want_loss, want_w, want_t, terms = _want(name, N)
    loss, gw, gt, _ = cos_loss_and_gradients(dec, pts, tgt)
    print(f"{name} N={N}: loss {float(loss):.8f} (float64 {want_loss:.8f}), |difference| {abs(float(loss) - want_loss):.3g}")
    assert abs(float(loss) - want_loss) <= 1e-5
    _check(dec, gw, gt, want_w, want_t, terms, f"{name} N={N} fused")
    assert bool((gt[want_t == 0] == 0).all())
    if N in (2081, R.LONG_N):
        loss2, gw2, _, _ = cos_loss_and_gradients(dec, pts, tgt)
        assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(gw, gw2))
    agw, agt = _autograd_gradients(dec, pts, tgt=tgt)
    _check(dec, agw, agt, want_w, want_t, terms, f"{name} N={N} autograd")


@pytest.mark.parametrize("name", R.EPS_LAYOUTS)
def test_eps_branches_and_scale_invariance_of_the_cosine_loss(name):
    """33 points whose targets hold one all-zero row, one of norm 1e-10 (both below the cosine's eps of 1e-8), one of norm 7 and one
    of norm 1e-3 (row 32, the second tile's only live row); the rest are unit.  Loss and gradients against float64
    torch.cosine_similarity(eps=1e-8) autograd with the bars of the float64 test.  The zero-target row contributes exactly nothing:
    the batch without it gives the same gradients once scaled by 32 / 33 to the same 1 / N.  Scaling every target row above eps by
    4 (a power of two) leaves loss and gradients within the bars of the unscaled run; with the row of norm 1e-10 scaled as well
    the device still follows float64 (below eps the clamped norm makes that row's term linear in the target, in the reference as
    on the device, so that row is not scale-invariant).  five160: O = 160, 20 columns per thread.
    Measured, worst ratio over weights and table: against float64 office_0 0.0016, five160 0.020 (all three target sets); targets
    x 4 against unscaled: 0, bit-identical; without the zero-target row: office_0 0.0019, five160 0.022, same non-zero entries."""
    from splatloc_amd.decoder import cos_loss_and_gradients
    dec, ref = _model(name)
    pts, unit = _batch(name, R.EPS_N)
    tgt = R.eps_targets(unit)
    res = {}
    for kind in ("eps", "eps_x4", "eps_x4_above"):
        t = tgt * R.eps_scale(kind)
        want_loss, want_w, want_t, terms = R.float64_gradients(ref, pts, t)
        loss, gw, gt, _ = cos_loss_and_gradients(dec, pts, t)
        print(f"{name} {kind}: loss {float(loss):.8f} (float64 {want_loss:.8f})")
        assert abs(float(loss) - want_loss) <= 1e-5
        _check(dec, gw, gt, want_w, want_t, terms, f"{name} {kind} fused")
        assert bool((gt[want_t == 0] == 0).all())
        agw, agt = _autograd_gradients(dec, pts, tgt=t)
        _check(dec, agw, agt, want_w, want_t, terms, f"{name} {kind} autograd")
        res[kind] = (loss, gw, gt, terms)
    loss, gw, gt, terms = res["eps"]
    loss4, gw4, gt4, _ = res["eps_x4_above"]
    assert abs(float(loss4) - float(loss)) <= 1e-5
    _check(dec, gw4, gt4, [g.double() for g in gw], gt.double(), terms, f"{name} targets x 4 against unscaled")
    keep = torch.arange(R.EPS_N) != R.EPS_ROWS["zero"]
    _, gwk, gtk, _ = cos_loss_and_gradients(dec, pts[keep], tgt[keep])
    scale = (R.EPS_N - 1) / R.EPS_N
    _check(dec, gw, gt, [g.double() * scale for g in gwk], gtk.double() * scale, terms, f"{name} without the zero-target row")
    assert torch.equal(gt != 0, gtk != 0)


@pytest.mark.parametrize("name", R.BOX_LAYOUTS)
def test_points_on_and_outside_the_box_in_the_backward(name):
    """The 33-point batch with four points replaced by the bound's two corners, a point 0.5 outside on every axis and a point on
    a face (each decided under float64).  Outside the box the cell index wraps as uint32; the fused encode of the forward and the
    scatter of the backward must agree on it: same bars, and the table gradient is non-zero exactly where float64's is.
    Measured, worst ratio: office_0 weights 0.0016, table 0.0014; three weights 0.00076, table 0.00045."""
    from splatloc_amd.decoder import cos_loss_and_gradients
    dec, ref = _model(name)
    base, tgt = _batch(name, R.BOX_N)
    pts = R.box_batch(ref, base)
    assert bool(ref.decided(pts).all())
    want_loss, want_w, want_t, terms = R.float64_gradients(ref, pts, tgt)
    loss, gw, gt, _ = cos_loss_and_gradients(dec, pts, tgt)
    assert abs(float(loss) - want_loss) <= 1e-5
    _check(dec, gw, gt, want_w, want_t, terms, f"{name} box fused")
    assert torch.equal(gt != 0, want_t != 0) and int((gt != 0).sum()) > 0
    agw, agt = _autograd_gradients(dec, pts, tgt=tgt)
    _check(dec, agw, agt, want_w, want_t, terms, f"{name} box autograd")
    assert torch.equal(agt != 0, want_t != 0)


def test_the_trainer_across_changing_batch_sizes():
    """One DecoderTrainer on `narrow` steps on fixed batches of 2081, 33, 2081 and 1 points, so it returns to a cached workspace
    after a smaller batch used another.  Each step's loss is, bit for bit, cos_loss_and_gradients' loss on a copy of the parameters
    as they were before that step (a fresh workspace every time), and after the four steps the parameters are within the bar of
    test_adam_matches_torch, 8 u (|p| + lr) per step taken, of torch.optim.Adam fed those gradients: nothing of a workspace of
    another N is left behind.
    Measured: the four losses identical; worst |trainer - torch Adam| / bar = 0.17 and 0.35 in two runs (the table gradient is an
    arrival-ordered scatter)."""
    from splatloc_amd.decoder import DecoderTrainer, cos_loss_and_gradients
    dec, probe = R.layout_decoder("narrow"), R.layout_decoder("narrow")
    ref = _model("narrow")[1]                          # the shared batches were drawn under the same initial parameters
    params = dec.feature_net.weights() + [dec.encoding.params]
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = torch.optim.Adam([{"params": twin[:-1], "weight_decay": 1e-6, "lr": LR}, {"params": twin[-1:], "eps": 1e-15, "lr": LR}],
                           betas=(0.9, 0.99))
    tr = DecoderTrainer(dec, lr=LR)
    assert bool(ref.decided(_batch("narrow", 2081)[0]).all())
    for k, n in enumerate(R.TRAINER_NS):
        pts, tgt = _batch("narrow", n)
        probe.load_state_dict(dec.state_dict())
        want_loss, gw, gt, _ = cos_loss_and_gradients(probe, pts, tgt)
        for p, g in zip(twin, gw + [gt]):
            p.grad = g.clone()
        opt.step()
        loss = tr.step(pts, tgt)
        print(f"step {k} (N = {n}): loss {float(loss):.8f}")
        assert torch.equal(loss, want_loss), (k, n, float(loss), float(want_loss))
        assert float(tr.w_grad.abs().sum()) == 0.0 and float(tr.t_grad.abs().sum()) == 0.0
    assert sorted(tr._buffers) == [1, 33, 2081]
    worst = 0.0
    for p, w in zip(params, twin):
        bar = len(R.TRAINER_NS) * 8 * R.U * (w.detach().abs().double() + LR)
        err = (p.detach().double() - w.detach().double()).abs()
        worst = max(worst, float((err / bar).max()))
        assert bool((err <= bar).all())
    print(f"parameters after {len(R.TRAINER_NS)} steps: worst |trainer - torch Adam| / bar = {worst:.3g}")
