"""Float64 restatement of FeatureDecoder for the decoder tests and the fixture generator (no test lives here).

`restated()` is the grid encoding's definition, the same as in tests/test_gpu_grid_encoding.py; `RestatedEncoding` wraps it as a
CPU-or-device module with tinycudann.Encoding's interface (float64 table, initialised exactly as
splatloc_amd.grid_encoding.Encoding(seed=1337) initialises its own); `RestatedDecoder` is the whole decoder in float64 with the
reference's state_dict keys, able to report every layer's pre-activation and the worst-case f32 rounding bar that goes with it."""
import os

import numpy as np
import torch

M32 = 0xFFFFFFFF
PRIMES = (1, 2654435761, 805459861)
OFFICE_0 = [[-3.0, 3.0], [-4.0, 2.5], [-2.0, 2.5]]     # configs/replica_nerf/office_0.yaml
U = 2.0 ** -24                                          # unit roundoff of f32


def office_0_config():
    return {"scene": {"bound": OFFICE_0, "voxel_sdf": 0.06},
            "decoder": {"enc": "HashGrid", "hidden_dim": 128, "num_layers": 4, "final_dim": 256}}


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative bound of a length-k f32 fma chain (or any-order sum of k terms)"""
    return k * U / (1.0 - k * U)


def restated(x, params, lay):
    """out [N, L*F] (float64) of the grid encoding for f32-valued points x [N, D] and a table `params` [n_params]"""
    D, F = lay.n_input_dims, lay.n_features_per_level
    x32 = x.detach().float()
    outs = []
    for lvl in range(lay.n_levels):
        scale, res, size, off = lay.scales[lvl], lay.resolutions[lvl], lay.sizes[lvl], lay.offsets[lvl]
        pos = (x32.double() * scale + 0.5).float()          # fmaf(scale, x, 0.5f): exact in f64, rounded to f32 once
        fl = torch.floor(pos)
        cell = fl.to(torch.int64) & M32
        frac = (pos - fl).double()
        acc = torch.zeros((x.shape[0], F), dtype=torch.float64, device=x.device)
        for c in range(1 << D):
            g = [(cell[:, d] + ((c >> d) & 1)) & M32 for d in range(D)]
            stride, index = 1, torch.zeros_like(g[0])
            for d in range(D):
                if stride <= size:
                    index = (index + g[d] * stride) & M32
                    stride = stride * res & M32
            if lay.grid_type == 0 and size < stride:
                index = torch.zeros_like(g[0])
                for d in range(D):
                    index = index ^ ((g[d] * PRIMES[d]) & M32)
            index = index % size
            w = torch.ones_like(frac[:, 0])
            for d in range(D):
                w = w * (frac[:, d] if (c >> d) & 1 else 1.0 - frac[:, d])
            rows = (off + index)[:, None] * F + torch.arange(F, device=x.device)[None, :]
            acc = acc + w[:, None] * params.double()[rows]
        outs.append(acc)
    return torch.cat(outs, 1)


class RestatedEncoding(torch.nn.Module):
    """tinycudann.Encoding's interface on the float64 restatement"""

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        super().__init__()
        from splatloc_amd.grid_encoding import GridLayout
        self.layout = GridLayout(n_input_dims, encoding_config)
        self.n_input_dims, self.n_output_dims = self.layout.n_input_dims, self.layout.n_output_dims
        gen = torch.Generator().manual_seed(int(seed))
        init = torch.rand((self.layout.n_params,), generator=gen, dtype=torch.float32).mul_(2e-4).sub_(1e-4)
        self.params = torch.nn.Parameter(init.double())

    def forward(self, x):
        return restated(x.to(self.params.device).float(), self.params, self.layout)


class RestatedDecoder(torch.nn.Module):
    """FeatureDecoder in float64 (the f64 bounding-box normalisation rounded once to f32, as Encoding's cast does), with the
    reference's parameter names.  Built from any decoder with `encoding.params`, `feature_net.model` and a layout."""

    def __init__(self, decoder, layout=None):
        super().__init__()
        self.layout = layout or (decoder.layout.grid if hasattr(decoder.layout, "grid") else decoder.layout)
        self.bounding_box = torch.as_tensor(decoder.bounding_box).detach().clone().double().cpu()
        self.encoding = torch.nn.Module()
        self.encoding.params = torch.nn.Parameter(decoder.encoding.params.detach().double().clone())
        self.feature_net = torch.nn.Module()
        layers = []
        for m in decoder.feature_net.model:
            if isinstance(m, torch.nn.Linear):
                lin = torch.nn.Linear(m.in_features, m.out_features, bias=False, dtype=torch.float64)
                lin.weight.data.copy_(m.weight.detach().double())
                layers.append(lin)
            else:
                layers.append(torch.nn.ReLU())
        self.feature_net.model = torch.nn.Sequential(*layers)
        self.to(decoder.encoding.params.device)

    def weights(self):
        return [m.weight for m in self.feature_net.model if isinstance(m, torch.nn.Linear)]

    def normalised(self, pos):
        bb = self.bounding_box
        pos = pos.detach().cpu().double()
        return ((pos - bb[:, 0]) / (bb[:, 1] - bb[:, 0])).float().to(self.encoding.params.device)

    def trace(self, pos):
        """(out, pre-activations per layer, bars per layer): bar = gamma_K * sum_k |a_k w_k| per element, the worst case of a
        length-K f32 fma chain on float64-exact inputs"""
        h = restated(self.normalised(pos), self.encoding.params, self.layout)
        pres, bars = [], []
        ws = self.weights()
        for l, w in enumerate(ws):
            pre = h @ w.t()
            pres.append(pre)
            bars.append(gamma(w.shape[1]) * (h.detach().abs() @ w.detach().abs().t()))
            h = torch.relu(pre) if l + 1 < len(ws) else pre
        return h / h.norm(dim=-1, keepdim=True), pres, bars

    def forward(self, pos):
        return self.trace(pos)[0]

    def decided(self, pos):
        """mask [N] of the points whose every hidden pre-activation is further from zero than its rounding bar: for the others an
        f32 evaluation may switch a ReLU the other way, which changes that point's gradient by far more than rounding"""
        with torch.no_grad():
            _, pres, bars = self.trace(pos)
        ok = torch.ones((pos.shape[0],), dtype=torch.bool, device=pres[0].device)
        for pre, bar in zip(pres[:-1], bars[:-1]):
            ok &= (pre.abs() > bar).all(dim=1)
        return ok


def cos_loss(out, gt):
    return 1 - torch.cosine_similarity(out, gt, dim=1).mean()


def reference_optimizer(dec, lr=1e-3):
    """train_decoder.py:48-51"""
    return torch.optim.Adam([{"params": dec.feature_net.parameters(), "weight_decay": 1e-6, "lr": lr},
                             {"params": dec.encoding.parameters(), "eps": 1e-15, "lr": lr}], betas=(0.9, 0.99))


def trained_scale_(decoder, seed=5):
    """values that mean something: a table of uniform(-1, 1) entries instead of the 1e-4 initialisation (in place)"""
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        p = decoder.encoding.params
        p.copy_((torch.rand(p.shape, generator=g) * 2 - 1).to(p.device))
    return decoder


def points_in_bound(n, seed, bound=OFFICE_0):
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(bound, dtype=torch.float64).unbind(1)
    return lo + torch.rand((n, 3), generator=g, dtype=torch.float64) * (hi - lo)      # CPU float64, as in train_decoder.py


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    """the decoder fixtures of tests/golden/make_golden_decoder.py as one dict"""
    out = {}
    for name in ("decoder.npz", "decoder_grads.npz", "decoder_step3.npz", "decoder_table3.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def fixture_config(fx):
    return {"scene": {"bound": fx["config_bound"].tolist(), "voxel_sdf": float(fx["config_voxel_sdf"])},
            "decoder": {"enc": str(fx["config_enc"]), "hidden_dim": int(fx["config_hidden_dim"]),
                        "num_layers": int(fx["config_num_layers"]), "final_dim": int(fx["config_final_dim"])}}


def decided_pool_batch(ref, k, n=256, pool=320, bound=OFFICE_0):
    """the fixture generator's batch rule for any model: the first n points of a fixed pool of uniform points (numpy
    default_rng(100 + k)) whose hidden pre-activations all lie outside their rounding bar of zero under `ref`; unit targets"""
    lo, hi = np.array(bound, np.float64).T
    pts = torch.from_numpy(lo + np.random.default_rng(100 + k).random((pool, 3)) * (hi - lo))
    pts = pts[ref.decided(pts).cpu()][:n]
    assert pts.shape[0] == n
    return pts, unit_targets(n, 256, 300 + k)


def targets(k, n=256, width=256):
    """targets of fixture batch k: elementwise numpy on default_rng draws (bit-identical everywhere), not normalised"""
    return (np.random.default_rng(200 + k).random((n, width)) - 0.5).astype(np.float32)


def unit_targets(n, width, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((n, width), generator=g)
    return t / t.norm(dim=-1, keepdim=True)
