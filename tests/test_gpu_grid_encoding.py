"""tinycudann.Encoding on the MI355X: forward and both gradients against a float64 torch restatement of the grid encoding
(tests/grid_encoding_reference.py, same host level table), the CPU-input path, a FeatureDecoder-shaped training loop and the
kernels' codegen."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from splatloc_amd import build as B
from tests.grid_encoding_reference import points as _points, restated

pytestmark = pytest.mark.gpu

OFFICE_0 = [[-3.0, 3.0], [-4.0, 2.5], [-2.0, 2.5]]     # configs/replica_nerf/office_0.yaml: desired resolution 108


def splatloc_config(desired=108, otype="HashGrid"):
    return {"otype": otype, "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
            "per_level_scale": float(np.exp2(np.log2(desired / 16) / 15))}


def _encoding(cfg, D=3, seed=1337):
    import tinycudann as tcnn
    enc = tcnn.Encoding(D, cfg, seed=seed, dtype=torch.float)
    with torch.no_grad():                                     # values that mean something
        g = torch.Generator().manual_seed(seed + 1)
        enc.params.copy_((torch.rand(enc.params.shape, generator=g) * 2 - 1).cuda())
    return enc


CASES = [("hash3", 3, splatloc_config()), ("dense2", 2, {"otype": "DenseGrid", "n_levels": 4, "n_features_per_level": 4,
                                                        "base_resolution": 8, "per_level_scale": 1.9}),
         ("tiled3", 3, {"otype": "Grid", "type": "Tiled", "n_levels": 5, "n_features_per_level": 1, "base_resolution": 6,
                        "per_level_scale": 1.6}),
         ("hash2_f8", 2, {"otype": "HashGrid", "n_levels": 20, "n_features_per_level": 8, "log2_hashmap_size": 12,
                          "base_resolution": 4, "per_level_scale": 1.5})]


@pytest.mark.parametrize("name,D,cfg", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("N", [1, 255, 256, 100_003])
def test_forward_matches_float64_restatement(name, D, cfg, N):
    enc = _encoding(cfg, D)
    lay = enc.layout
    if name == "hash3":
        hashed = [r ** 3 > s for r, s in zip(lay.resolutions, lay.sizes)]
        assert any(hashed) and not all(hashed)                # dense and hashed levels both covered
    x = _points(N, 11 + N, lay).cuda()
    out = enc(x)
    assert out.shape == (N, lay.n_output_dims) and out.dtype == torch.float32
    ref, sabs = restated(x, enc.params.detach(), lay)
    err = (out.double() - ref).abs()
    bar = 4 * 2.0 ** -23 * sabs
    assert bool((err <= bar).all()), (name, N, float((err - bar).max()))


def test_empty_batch():
    enc = _encoding(splatloc_config())
    out = enc(torch.zeros((0, 3), device="cuda"))
    assert out.shape == (0, 32)
    out.sum().backward()
    assert enc.params.grad is not None and float(enc.params.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("name,D,cfg", CASES, ids=[c[0] for c in CASES])
def test_parameter_gradient_matches_autograd(name, D, cfg):
    N = 20_001
    enc = _encoding(cfg, D)
    lay = enc.layout
    x = _points(N, 5, lay).cuda()
    G = torch.randn((N, lay.n_output_dims), generator=torch.Generator().manual_seed(3)).cuda()
    enc(x).backward(G)
    got = enc.params.grad.double()
    p64 = enc.params.detach().double().requires_grad_(True)
    ref, _ = restated(x, p64, lay)
    (ref * G.double()).sum().backward()
    p_abs = p64.detach().clone().requires_grad_(True)        # sum of |terms| per entry: the weights are >= 0
    ref_abs, _ = restated(x, p_abs, lay)
    (ref_abs * G.double().abs()).sum().backward()
    sabs = p_abs.grad
    untouched = sabs == 0
    assert bool((got[untouched] == 0).all())
    assert bool(((got - p64.grad).abs() <= 1e-5 * sabs).all()), float(((got - p64.grad).abs() - 1e-5 * sabs).max())
    assert int((~untouched).sum()) > 0


@pytest.mark.parametrize("name,D,cfg", CASES, ids=[c[0] for c in CASES])
def test_input_gradient_matches_autograd(name, D, cfg):
    N = 4099
    enc = _encoding(cfg, D)
    lay = enc.layout
    x = (torch.rand((N, D), generator=torch.Generator().manual_seed(9)) * 0.98 + 0.01).cuda()   # generic points, off the faces
    G = torch.randn((N, lay.n_output_dims), generator=torch.Generator().manual_seed(4)).cuda()
    xg = x.clone().requires_grad_(True)
    enc(xg).backward(G)
    x64 = x.double().requires_grad_(True)
    ref, _, bound = restated(x64, enc.params.detach(), lay, want_x_grad=True, G=G)
    (ref * G.double()).sum().backward()
    err = (xg.grad.double() - x64.grad).abs()
    assert bool((err <= 1e-5 * bound).all()), float((err / bound).max())
    assert float(x64.grad.abs().max()) > 0


def test_cpu_float64_input_warns_and_matches_gpu_f32():
    enc = _encoding(splatloc_config())
    x = _points(1000, 21, enc.layout).double()
    with pytest.warns(UserWarning, match="ROCm device"):
        out_cpu = enc(x)
    assert out_cpu.is_cuda and out_cpu.dtype == torch.float32
    out_gpu = enc(x.float().cuda())
    assert torch.equal(out_cpu, out_gpu)


class _Decoder(torch.nn.Module):
    """FeatureDecoder's shape: bounding-box normalisation -> Encoding -> 4 bias-free Linear layers (128 hidden -> 256) ->
    unit normalisation.  The encoding is the HIP module or the float64 restatement; the MLP runs in its own dtype."""

    def __init__(self, bound, encoding, activation=torch.nn.ReLU):
        super().__init__()
        self.bounding_box = torch.tensor(bound, dtype=torch.float64)
        self.encoding = encoding
        dims = [encoding.n_output_dims, 128, 128, 128, 256]
        layers = []
        for i in range(4):
            layers.append(torch.nn.Linear(dims[i], dims[i + 1], bias=False))
            if i < 3:
                layers.append(activation())
        self.feature_net = torch.nn.Sequential(*layers)

    def forward(self, pos):
        pos = (pos - self.bounding_box[:, 0]) / (self.bounding_box[:, 1] - self.bounding_box[:, 0])
        f = self.feature_net(self.encoding(pos).cuda().to(self.feature_net[0].weight.dtype))
        return f / f.norm(dim=-1, keepdim=True)


class _RestatedEncoding(torch.nn.Module):
    def __init__(self, enc):
        super().__init__()
        self.layout = enc.layout
        self.n_output_dims = enc.n_output_dims
        self.params = torch.nn.Parameter(enc.params.detach().double().clone())

    def forward(self, x):
        self.last_x = x.float().cuda()
        self.last_out = restated(self.last_x, self.params, self.layout)[0]
        self.last_out.retain_grad()
        return self.last_out

    def conditioning(self):
        """per entry, sum of |terms| / |sum| of the last backward's parameter gradient (0 where nothing contributed)"""
        p_abs = torch.zeros_like(self.params, requires_grad=True)
        (restated(self.last_x, p_abs, self.layout)[0] * self.last_out.grad.abs()).sum().backward()
        return torch.where(p_abs.grad > 0, p_abs.grad / self.params.grad.abs(), torch.zeros_like(p_abs.grad))


def _optimizer(dec):
    return torch.optim.Adam([{"params": dec.feature_net.parameters(), "weight_decay": 1e-6, "lr": 1e-3},
                             {"params": dec.encoding.parameters(), "eps": 1e-15, "lr": 1e-3}], betas=(0.9, 0.99))


def _data():
    g = torch.Generator().manual_seed(1)
    lo, hi = torch.tensor(OFFICE_0, dtype=torch.float64).unbind(1)
    pts = lo + torch.rand((1024, 3), generator=g, dtype=torch.float64) * (hi - lo)       # CPU float64, as in train_decoder.py
    tgt = torch.randn((1024, 256), generator=g)
    tgt = (tgt / tgt.norm(dim=-1, keepdim=True)).cuda()
    return g, pts, tgt


def _step(dec, opt, xb, tb):
    loss = (1.0 - (dec(xb) * tb.to(dec.feature_net[0].weight.dtype)).sum(-1)).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss)


def test_feature_decoder_first_steps_match_float64_restatement():
    """Three Adam steps of the same loop on the encoding group, HIP encoding against the float64 restatement, through one
    fixed float64 MLP with tanh in place of ReLU: the encoding is the only difference.  (Training the MLP as well would compare
    the optimiser, not the encoding: Adam's first step moves every MLP weight by about +-lr whatever its gradient's size, so a
    weight whose tiny gradient differs in sign between the two paths ends up 2 lr apart.  A ReLU whose pre-activation lies within
    rounding of 0 is on in one path and off in the other, which changes that point's dL/dout by up to 1e-3 relative.)
    Bar: 1e-4 of (|parameter| + 3 lr), the reach of three Adam steps: Adam with eps 1e-15 normalises each entry's gradient, so
    a relative error of dL/dout becomes that relative error of every update of about lr, and a parameter whose initial value
    and updates nearly cancel would otherwise be held to far less than its steps; the f32 encoding output's rounding reaches
    dL/dout through the bias-free MLP and the unit normalisation amplified to about 1e-5.  Plus lr * 1e-6 * kappa per entry,
    kappa = the largest sum |terms| / |gradient| of the three steps (contributions to an entry that cancel)."""
    import tinycudann as tcnn
    torch.manual_seed(0)
    dec = _Decoder(OFFICE_0, tcnn.Encoding(3, splatloc_config(), dtype=torch.float), torch.nn.Tanh)
    dec.feature_net.double()
    dec.cuda()
    ref = _Decoder(OFFICE_0, _RestatedEncoding(dec.encoding), torch.nn.Tanh)
    ref.feature_net.load_state_dict(dec.feature_net.state_dict())
    ref.cuda()
    for d in (dec, ref):
        d.feature_net.requires_grad_(False)
    g, pts, tgt = _data()
    opt, opt_ref = [torch.optim.Adam([{"params": d.encoding.parameters(), "eps": 1e-15, "lr": 1e-3}], betas=(0.9, 0.99))
                    for d in (dec, ref)]
    kappa = torch.zeros_like(ref.encoding.params)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)           # the CPU-input warning, once per step
        for _ in range(3):
            sel = torch.randint(0, 1024, (256,), generator=g)
            xb, tb = pts[sel], tgt[sel.cuda()]
            loss, loss_ref = _step(dec, opt, xb, tb), _step(ref, opt_ref, xb, tb)
            assert abs(loss - loss_ref) <= 1e-5
            kappa = torch.maximum(kappa, ref.encoding.conditioning())
            got, want = dec.encoding.params.detach().double(), ref.encoding.params.detach()
            bar = 1e-4 * (want.abs() + 3e-3) + 1e-3 * 1e-6 * kappa
            ratio = float(((got - want).abs() / bar).max())
            print(f"worst |HIP - float64| / bar: {ratio:.3g}")
            assert ratio <= 1.0
            assert int((kappa > 0).sum()) > 0


def test_feature_decoder_loop_trains_and_round_trips():
    import tinycudann as tcnn
    torch.manual_seed(0)
    cfg = splatloc_config()
    dec = _Decoder(OFFICE_0, tcnn.Encoding(3, cfg, dtype=torch.float)).cuda()
    g, pts, tgt = _data()
    opt = _optimizer(dec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        losses = []
        for _ in range(200):
            sel = torch.randint(0, 1024, (256,), generator=g)
            losses.append(_step(dec, opt, pts[sel], tgt[sel.cuda()]))
        assert np.mean(losses[-20:]) < np.mean(losses[:20]) - 0.05, (losses[:3], losses[-3:])
        sd = dec.state_dict()
        assert "encoding.params" in sd and sd["encoding.params"].shape == (5_724_048,)
        fresh = _Decoder(OFFICE_0, tcnn.Encoding(3, cfg, seed=7, dtype=torch.float)).cuda()
        fresh.load_state_dict(sd)
        with torch.no_grad():
            assert torch.equal(fresh(pts[:1000]), dec(pts[:1000]))


def _usage(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in B._flags(src) if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def test_grid_encoding_kernels_use_no_scratch():
    u = _usage("grid_encoding.hip")
    kernels = {k: v for k, v in u.items() if "grid_encode_" in k}
    assert len(kernels) == 8 + 8 * 3, sorted(kernels)         # forward + 3 backward variants for D {2,3} x F {1,2,4,8}
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
