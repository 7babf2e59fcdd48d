"""The fused FeatureDecoder on the MI355X: encoding bits, per-layer rounding bounds, end-to-end error against the composed path,
gradients, Adam, the first reference steps, the training loop, checkpoints both ways and the matching pipeline."""
import warnings

import numpy as np
import pytest
import torch

from tests import decoder_reference as R

pytestmark = pytest.mark.gpu

LR = 1e-3


def _decoder(seed=0, trained=False, cfg=None):
    from splatloc_amd.decoder import FeatureDecoder
    torch.manual_seed(seed)
    dec = FeatureDecoder(cfg or R.office_0_config()).cuda()
    return R.trained_scale_(dec) if trained else dec


class _Composed(torch.nn.Module):
    """the composed path: tinycudann.Encoding + torch layers, with the reference's module names (so checkpoints load)"""

    def __init__(self, fused):
        super().__init__()
        import tinycudann as tcnn
        from splatloc_amd.decoder import FeatureNet, _encoding_config
        self.bounding_box = fused.bounding_box
        self.encoding = tcnn.Encoding(3, _encoding_config(fused.config["decoder"]["enc"], fused.resolution_sdf), dtype=torch.float)
        d = fused.layout.dims
        self.feature_net = FeatureNet(d[0], d[1], len(d) - 1, d[-1])
        self.load_state_dict(fused.state_dict())
        self.cuda()

    def forward(self, pos):
        pos = (pos - self.bounding_box[:, 0]) / (self.bounding_box[:, 1] - self.bounding_box[:, 0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            f = self.feature_net.model(self.encoding(pos).cuda())
        return f / f.norm(dim=-1, keepdim=True)


def _training_forward(dec, pts):
    from splatloc_amd import decoder as D
    dev = dec.encoding.params.device
    x = D._points(pts, dev)
    N = int(x.shape[0])
    acts = dec.layout.activation_buffer(N, dev)
    out = D._launch_forward(dec.layout, x, dec.encoding.params.data, [w.data for w in dec.feature_net.weights()], acts)
    return out, dec.layout.split_activations(acts, N)


def test_encoded_features_are_bit_identical_to_the_encoding():
    import tinycudann as tcnn
    from splatloc_amd.decoder import _encoding_config
    dec = _decoder(trained=True)
    enc = tcnn.Encoding(3, _encoding_config("HashGrid", dec.resolution_sdf), dtype=torch.float)
    with torch.no_grad():
        enc.params.copy_(dec.encoding.params)
    pts = R.points_in_bound(5000, 3)
    pts[:4] = torch.tensor([[-3.0, -4.0, -2.0], [3.0, 2.5, 2.5], [-3.5, 3.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    bb = dec.bounding_box
    xn = ((pts - bb[:, 0]) / (bb[:, 1] - bb[:, 0])).float().cuda()
    _, rec = _training_forward(dec, pts)
    assert torch.equal(rec["xn"], xn)
    with torch.no_grad():
        assert torch.equal(rec["inputs"][0], enc(xn))
    # a device f32 input is widened exactly
    _, rec32 = _training_forward(dec, pts.float().cuda())
    xn32 = ((pts.float().double() - bb[:, 0]) / (bb[:, 1] - bb[:, 0])).float().cuda()
    assert torch.equal(rec32["xn"], xn32)


@pytest.mark.parametrize("trained", [False, True], ids=["initial", "trained_scale"])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 5000, 40000])
def test_layers_within_the_fma_chain_bound(N, trained):
    """Each layer is recomputed in float64 FROM THE DEVICE'S OWN input activations.  The device's pre-activation is a length-K
    f32 fma chain, so it lies within gamma_K * sum_k |a_k w_k| of the exact value (gamma_K = K u / (1 - K u), u = 2^-24); ReLU
    is 1-Lipschitz, so the stored post-ReLU activation meets the same bar.
    Unit normalisation, out = f / sqrtf(s), s = the f32 sum of the 256 squares in any order: every square carries one rounding
    and the sum at most 255 more, so s = S (1 + d1) with |d1| <= gamma_256 and S the exact sum of squares of the device's f;
    sqrtf and the division are correctly rounded (one u each), hence out = f / sqrt(S) * (1 + d1)^(-1/2) (1 + d2)(1 + d3) and
    |out - f / sqrt(S)| <= (gamma_256 / 2 + 3 u) |f| / sqrt(S): the third u absorbs every second-order term.  The stored norm
    meets (gamma_256 / 2 + 2 u) sqrt(S).  N = 40000 runs the 64-point tiles, the others the 32-point tiles; that the two tile
    heights give the same bits is tests/test_gpu_decoder_edges.py::test_tile_heights_give_the_same_bits."""
    dec = _decoder(trained=trained)
    pts = R.points_in_bound(N, 100 + N)
    out, rec = _training_forward(dec, pts)
    assert out.shape == (N, 256) and out.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(dec(pts), out)                     # inference kernel path, same bits
    if N == 0:
        return
    ws = [w.detach().double() for w in dec.feature_net.weights()]
    for l, w in enumerate(ws):
        a = rec["inputs"][l].double()
        pre = a @ w.t()
        bar = R.gamma(w.shape[1]) * (a.abs() @ w.abs().t())
        got = (rec["inputs"][l + 1] if l + 1 < len(ws) else rec["f"]).double()
        want = torch.relu(pre) if l + 1 < len(ws) else pre
        excess = float(((got - want).abs() - bar).max())
        print(f"N={N} layer {l}: worst |device - f64| / bar = {float(((got - want).abs() / bar.clamp_min(1e-300)).max()):.3g}")
        assert excess <= 0.0, (l, excess)
    f = rec["f"].double()
    n64 = f.norm(dim=-1, keepdim=True)
    nbar = R.gamma(256) / 2
    assert bool(((rec["norm"].double()[:, None] - n64).abs() <= (nbar + 2 * R.U) * n64).all())
    assert bool(((out.double() - f / n64).abs() <= (nbar + 3 * R.U) * (f / n64).abs()).all())


def _errors(fused, pts):
    """(fused error, composed error, fused output): max |out - float64| over the batch"""
    ref = R.RestatedDecoder(fused)
    comp = _Composed(fused)
    with torch.no_grad():
        want = ref(pts)
        got_f, got_c = fused(pts), comp(pts)
    return float((got_f.double() - want).abs().max()), float((got_c.double() - want).abs().max()), got_f


@pytest.mark.parametrize("trained", [False, True], ids=["initial", "trained_scale"])
def test_end_to_end_error_against_the_composed_path(trained):
    """Both paths are f32 chains of the same lengths in different orders; the fused error against float64 may be at most 4 x the
    composed path's own error (the fused chain is strictly sequential, a blocked GEMM is not).  Measured on the MI355X (max abs
    error over three 256-point batches): fused 0.93e-7 .. 1.06e-7, composed 0.86e-7 .. 1.04e-7."""
    dec = _decoder(trained=trained)
    for seed in (1, 2, 3):
        pts = R.points_in_bound(256, seed)
        e_f, e_c, _ = _errors(dec, pts)
        print(f"end to end, batch {seed}: fused {e_f:.3g}, composed {e_c:.3g}")
        assert e_f <= 4 * e_c


def _row_bar_ok(got, want, what):
    """the project's gradient bar: rtol 1e-4 plus 1e-3 of the row's own maximum"""
    got, want = got.double().reshape(want.shape[0], -1), want.double().reshape(want.shape[0], -1)
    bar = 1e-4 * want.abs() + 1e-3 * want.abs().max(dim=1, keepdim=True).values
    ratio = float(((got - want).abs() / bar.clamp_min(1e-300)).max())
    print(f"{what}: worst |got - want| / bar = {ratio:.3g}")
    assert bool(((got - want).abs() <= bar).all()), (what, ratio)


def _level_rows(dec, g):
    """the table gradient as one row per level"""
    lay = dec.layout.grid
    F = lay.n_features_per_level
    return [g[o * F:(o + s) * F] for o, s in zip(lay.offsets, lay.sizes)]


def _fixture_decoder(fx):
    """the fused decoder as the reference constructed its own: office_0 configuration, torch.manual_seed(0)"""
    dec = _decoder(seed=0, cfg=R.fixture_config(fx))
    for i, w in enumerate(dec.feature_net.weights()):
        assert torch.equal(w.detach().cpu(), torch.from_numpy(fx[f"w0_{i}"]))       # nn.Linear's initialisation under the seed
    return dec


def _dense_table(dec, idx, val):
    g = torch.zeros((dec.encoding.params.numel() // 2, 2), dtype=torch.float64)
    g[torch.from_numpy(idx.astype(np.int64))] = torch.from_numpy(val).double()
    return g.view(-1).cuda()


def test_fixture_step_1_outputs_against_the_composed_path():
    """The reference's own float64 outputs of step 1 (tests/golden/decoder.npz).  Both paths are f32 chains of the same lengths in
    different orders; the fused error may be at most 4 x the composed path's own error against the same values."""
    fx = R.fixture()
    dec = _fixture_decoder(fx)
    comp = _Composed(dec)
    pts = torch.from_numpy(fx["batches"][0])
    want = torch.from_numpy(fx["outputs"]).cuda()
    with torch.no_grad():
        e_f = float((dec(pts).double() - want).abs().max())
        e_c = float((comp(pts).double() - want).abs().max())
    print(f"fixture step 1: fused {e_f:.3g}, composed {e_c:.3g}")
    assert e_f <= 4 * e_c


@pytest.mark.parametrize("case", ["fixture", "trained_scale"])
def test_gradients_match_float64(case):
    """cos_loss gradients per gradient row (a weight's output row; a level of the table) with the project's bar.  `fixture`: the
    reference's own step-1 loss and gradients (tests/golden/decoder_grads.npz) on the fixture's first batch, whose points all
    have decided ReLUs (the generator's batch rule; the share of excluded points in the batch is 0 <= 1 %).  `trained_scale`:
    float64 autograd of the restatement on a table of uniform(-1, 1) entries, on a batch made by the same rule.  The autograd
    route (forward + cos_loss + .backward()) meets the same bar, and the MLP weight gradients of two identical calls are
    bit-identical."""
    from splatloc_amd.decoder import cos_loss, cos_loss_and_gradients
    if case == "fixture":
        fx = R.fixture()
        dec = _fixture_decoder(fx)
        pts, tgt = torch.from_numpy(fx["batches"][0]), torch.from_numpy(R.targets(0))
        assert bool(R.RestatedDecoder(dec).decided(pts).all())
        want_loss = float(fx["losses"][0])
        want_w = [torch.from_numpy(fx[f"dw_{i}"]).double().cuda() for i in range(4)]
        want_t = _dense_table(dec, fx["dtable_idx"], fx["dtable_val"])
    else:
        dec = _decoder(trained=True)
        ref = R.RestatedDecoder(dec)
        pts, tgt = R.decided_pool_batch(ref, 7)
        loss64 = R.cos_loss(ref(pts), tgt.cuda().double())
        loss64.backward()
        want_loss, want_w, want_t = float(loss64), [w.grad for w in ref.weights()], ref.encoding.params.grad
    loss, gw, gt, _ = cos_loss_and_gradients(dec, pts, tgt)
    print(f"loss {float(loss):.8f} (float64 {want_loss:.8f})")
    assert abs(float(loss) - want_loss) <= 1e-5
    for l, (g, w) in enumerate(zip(gw, want_w)):
        _row_bar_ok(g, w, f"fused dW{l}")
    for lvl, (g, w) in enumerate(zip(_level_rows(dec, gt), _level_rows(dec, want_t))):
        _row_bar_ok(g[None], w[None], f"fused dtable level {lvl}")
    assert bool((gt[want_t == 0] == 0).all())
    loss2, gw2, _, _ = cos_loss_and_gradients(dec, pts, tgt)
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(gw, gw2))
    # autograd route
    dec.zero_grad()
    cos_loss(dec(pts), tgt.cuda()).backward()
    for l, (w, w64) in enumerate(zip(dec.feature_net.weights(), want_w)):
        _row_bar_ok(w.grad, w64, f"autograd dW{l}")
    for lvl, (g, w) in enumerate(zip(_level_rows(dec, dec.encoding.params.grad), _level_rows(dec, want_t))):
        _row_bar_ok(g[None], w[None], f"autograd dtable level {lvl}")


def test_empty_batch_and_zero_row():
    dec = _decoder()
    out = dec(torch.zeros((0, 3), dtype=torch.float64))
    assert out.shape == (0, 256)
    out.sum().backward()
    assert float(dec.encoding.params.grad.abs().sum()) == 0.0
    assert all(float(w.grad.abs().sum()) == 0.0 for w in dec.feature_net.weights())
    with torch.no_grad():                                         # a zero output row is 0 / 0 = NaN, as in the reference
        dec.feature_net.weights()[-1].zero_()
        assert bool(torch.isnan(dec(R.points_in_bound(3, 1))).all())


def test_requesting_the_input_gradient_raises():
    dec = _decoder()
    pts = R.points_in_bound(8, 2).float().cuda().requires_grad_(True)
    with pytest.raises(ValueError, match="gradient with respect to the points"):
        dec(pts)
    with torch.no_grad():
        assert dec(pts).shape == (8, 256)            # nothing is requested when no graph is recorded


def _adam_reference(params, grads, steps, zero_after_first=False):
    ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = torch.optim.Adam([{"params": ps[:-1], "weight_decay": 1e-6, "lr": LR}, {"params": ps[-1:], "eps": 1e-15, "lr": LR}],
                           betas=(0.9, 0.99))
    for k in range(steps):
        for p, g in zip(ps, grads):
            p.grad = torch.zeros_like(g) if (zero_after_first and k > 0) else g.clone()
        opt.step()
    return [p.detach() for p in ps]


@pytest.mark.parametrize("steps,zero_after_first", [(1, False), (3, False), (3, True)], ids=["one", "three", "momentum_only"])
def test_adam_matches_torch(steps, zero_after_first):
    """splatraster_decoder_adam against torch.optim.Adam with the reference's two groups on the same gradients: parameters within
    8 * 2^-24 * (|p| + lr), a few f32 roundings of an update of size about lr.  With zero gradients after the first step every
    touched entry still moves through its momentum, and the gradient buffers are zero after every call."""
    from splatloc_amd.decoder import DecoderTrainer, cos_loss_and_gradients
    dec = _decoder(trained=True)
    pts, tgt = R.points_in_bound(256, 7), R.unit_targets(256, 256, 8)
    _, gw, gt, _ = cos_loss_and_gradients(dec, pts, tgt)
    params = dec.feature_net.weights() + [dec.encoding.params]
    before = [p.detach().clone() for p in params]
    want = _adam_reference(params, gw + [gt], steps, zero_after_first)
    tr = DecoderTrainer(dec, lr=LR)
    import ctypes as C
    from splatloc_amd import _native
    from splatloc_amd import decoder as D
    from splatloc_amd.rasterizer import _stream
    for k in range(steps):
        if not (zero_after_first and k > 0):
            tr.w_grad.copy_(torch.cat([g.reshape(-1) for g in gw]))
            tr.t_grad.copy_(gt)
        tr.steps += 1
        ws = [w.data for w in tr.weights]
        _native.check(_native.load().splatraster_decoder_adam(
            C.byref(dec.layout.native), D._pointer_array(ws), C.c_void_p(tr.w_grad.data_ptr()), C.c_void_p(tr.w_m.data_ptr()),
            C.c_void_p(tr.w_v.data_ptr()), C.c_void_p(tr.table.data_ptr()), C.c_void_p(tr.t_grad.data_ptr()),
            C.c_void_p(tr.t_m.data_ptr()), C.c_void_p(tr.t_v.data_ptr()), tr.steps, LR, LR, 0.9, 0.99, 1e-8, 1e-15, 1e-6,
            _stream(tr.table.device)), "decoder_adam")
        assert float(tr.w_grad.abs().sum()) == 0.0 and float(tr.t_grad.abs().sum()) == 0.0
    for p, w, b in zip(params, want, before):
        bar = 8 * R.U * (w.abs().double() + LR)
        assert bool(((p.detach().double() - w.double()).abs() <= bar).all())
    touched = gt != 0
    moved = (dec.encoding.params.detach() - before[-1]).abs()
    assert int(touched.sum()) > 0 and bool((moved[touched] > 0.5 * LR).all()) and float(moved[~touched].max()) == 0.0
    sd = tr.state_dict()
    assert len(sd["state"]) == 5 and sd["param_groups"][1]["eps"] == 1e-15 and float(sd["state"][4]["step"]) == steps
    torch_opt = R.reference_optimizer(dec)
    torch_opt.load_state_dict(sd)                                 # the exported state is torch.optim.Adam's own format


def test_first_three_reference_steps():
    """Three steps of DecoderTrainer on the fixture's three batches against what the reference's own FeatureDecoder, cos_loss and
    optimiser produced (tests/golden/decoder*.npz).  Losses within 1e-5.  Parameters after step 3 within 1e-4 * (|p| + 3 lr), the
    reach of three Adam steps: Adam normalises each entry's gradient, so a relative error of the gradient becomes that relative
    error of an update of about lr, and a parameter whose value and updates nearly cancel would otherwise be held to far less
    than its steps.  Plus lr * 1e-6 * kappa per entry, kappa = the largest sum |per-point terms| / |gradient| of the three steps:
    contributions to an entry that cancel leave a gradient whose f32 rounding is that much larger relative to it (for a weight
    the terms are dPre[p][o] * H[p][k] over the points p; for a table entry the corner contributions).  kappa comes from the
    float64 restatement run alongside under torch.optim.Adam.  It is used for that ratio alone, to about one significant digit; it
    must reproduce the fixture's losses to 1e-8, three orders below the bar the device is held to, which shows it is the same model
    on the same data (the device's float64 kernels and the CPU's sum in different orders; measured difference 1.3e-10)."""
    from splatloc_amd.decoder import DecoderTrainer
    fx = R.fixture()
    dec = _fixture_decoder(fx)
    ref = R.RestatedDecoder(dec)
    opt = R.reference_optimizer(ref, LR)
    tr = DecoderTrainer(dec, lr=LR)
    kappa = [torch.zeros_like(p) for p in ref.weights() + [ref.encoding.params]]
    for k in range(3):
        pts, tgt = torch.from_numpy(fx["batches"][k]), torch.from_numpy(R.targets(k))
        out, pres, _ = ref.trace(pts)
        for p in pres:
            p.retain_grad()
        loss64 = R.cos_loss(out, tgt.cuda().double())
        assert abs(float(loss64) - float(fx["losses"][k])) <= 1e-8
        opt.zero_grad()
        loss64.backward()
        # conditioning of every gradient entry
        with torch.no_grad():
            h = R.restated(ref.normalised(pts), ref.encoding.params, ref.layout)
            for l, w in enumerate(ref.weights()):
                terms = pres[l].grad.abs().t() @ h.abs()
                kappa[l] = torch.maximum(kappa[l], torch.where(w.grad != 0, terms / w.grad.abs(), torch.zeros_like(terms)))
                h = torch.relu(pres[l])
        p_abs = torch.zeros_like(ref.encoding.params, requires_grad=True)
        d_enc = (pres[0].grad @ ref.weights()[0].detach()).abs()
        (R.restated(ref.normalised(pts), p_abs, ref.layout) * d_enc).sum().backward()
        g = ref.encoding.params.grad
        kappa[-1] = torch.maximum(kappa[-1], torch.where(g != 0, p_abs.grad / g.abs(), torch.zeros_like(g)))
        opt.step()
        loss = tr.step(pts, tgt)
        print(f"step {k}: loss {float(loss):.7f} (reference {float(fx['losses'][k]):.7f})")
        assert abs(float(loss) - float(fx["losses"][k])) <= 1e-5
    idx = torch.from_numpy(fx["table3_idx"].astype(np.int64)).cuda()
    got = [w.detach().double() for w in dec.feature_net.weights()] + [dec.encoding.params.detach().double().view(-1, 2)[idx]]
    want = [torch.from_numpy(fx[f"w3_{i}"]).double().cuda() for i in range(4)] + [torch.from_numpy(fx["table3_val"]).double().cuda()]
    kaps = kappa[:-1] + [kappa[-1].view(-1, 2)[idx]]
    for name, p, w, kap in zip(["W0", "W1", "W2", "W3", "table"], got, want, kaps):
        bar = 1e-4 * (w.abs() + 3 * LR) + LR * 1e-6 * kap
        ratio = float(((p - w).abs() / bar).max())
        print(f"{name}: worst |fused - reference| / bar = {ratio:.3g}")
        assert ratio <= 1.0, name
    # entries no batch touched have not moved
    init = torch.rand((dec.encoding.params.numel(),), generator=torch.Generator().manual_seed(1337)).mul_(2e-4).sub_(1e-4).cuda()
    mask = torch.ones((init.numel() // 2,), dtype=torch.bool, device="cuda")
    mask[idx] = False
    assert torch.equal(dec.encoding.params.detach().view(-1, 2)[mask], init.view(-1, 2)[mask])


def test_training_loop_trains_and_checkpoints_travel():
    from splatloc_amd.decoder import FeatureDecoder, train_decoder
    dec = _decoder()
    pts, tgt = R.points_in_bound(1000, 1), R.unit_targets(1000, 256, 2)      # 1000 = 3 * 256 + 232: a short last batch
    losses = train_decoder(dec, pts, tgt, num_epochs=50, batch_size=256, lr=LR, seed=0)
    assert losses.is_cuda and losses.shape == (200,)
    ls = losses.cpu().numpy()
    assert np.isfinite(ls).all()
    assert ls[-20:].mean() < ls[:20].mean() - 0.05, (ls[:3], ls[-3:])
    # a caller-supplied order is replayed exactly
    a, b = _decoder(seed=3), _decoder(seed=3)
    perms = [torch.randperm(1000, generator=torch.Generator().manual_seed(9)) for _ in range(2)]
    la = train_decoder(a, pts, tgt, num_epochs=2, permutations=perms)
    lb = train_decoder(b, pts, tgt, num_epochs=2, permutations=perms)
    assert la.shape == (8,) and torch.equal(la[:1], lb[:1])
    # state_dict round trips: into a fresh fused decoder (same bits) and into the composed module (end-to-end bar)
    sd = dec.state_dict()
    assert list(sd) == ["encoding.params"] + [f"feature_net.model.{i}.weight" for i in (0, 2, 4, 6)]
    fresh = _decoder(seed=11)
    fresh.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(fresh(pts), dec(pts))
    e_f, e_c, _ = _errors(dec, pts[:256])
    print(f"trained checkpoint: fused {e_f:.3g}, composed {e_c:.3g}")
    assert e_f <= 4 * e_c
    assert isinstance(fresh, FeatureDecoder)


def test_pipeline_matches_are_the_same_with_either_decoder():
    from splatloc_amd import matching as M
    from tests.test_gpu_matching import _frame
    from tests.test_host_matching import golden
    g = golden()
    W, H = (int(x) for x in g["f_size"])
    cfg = R.office_0_config()
    cfg["scene"] = {"bound": [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]], "voxel_sdf": 0.06}      # the fixture's room
    fused = _decoder(trained=True, cfg=cfg)
    comp = _Composed(fused)
    args = (torch.from_numpy(g["f_points"]).cuda(), torch.from_numpy(g["f_marker"]), _frame(g), g["f_K"], W, H)
    with torch.no_grad():
        p3a, fa, _ = M.get_frusm_pts(*args, decoder=fused)
        p3b, fb, _ = M.get_frusm_pts(*args, decoder=comp)
    assert np.array_equal(p3a, p3b) and fa.shape == (len(p3a), 256) and len(p3a) > 50
    rng = np.random.default_rng(4)
    pick = rng.permutation(len(p3a))[: len(p3a) // 2]
    query = fb[pick].t().contiguous() + 0.02 * torch.from_numpy(rng.standard_normal((256, len(pick))).astype(np.float32)).cuda()
    ma, _ = M.hungarian_solve(query, fa.t().contiguous())
    mb, _ = M.hungarian_solve(query, fb.t().contiguous())
    assert ma.shape[1] > 0 and torch.equal(ma, mb)
