"""FeatureDecoder (models/decoders.py:43-68) and its training loop (train_decoder.py:20-25,48-51,64-82) on the fused HIP kernels.

`FeatureDecoder(config)` replaces the reference's class with a one-line import change: same config keys, same `state_dict` keys
and shapes (`encoding.params`, `feature_net.model.{0,2,...}.weight`), so checkpoints travel both ways.  The forward is ONE launch
(bounding-box normalisation, grid encoding, the bias-free ReLU MLP on f32 MFMA, unit normalisation: csrc/decoder.hip); it is
differentiable with respect to the parameters through `_DecoderFunction`.  `DecoderTrainer.step` is forward + cosine loss + backward
+ Adam over both parameter groups in five launches with no host synchronisation.  Shapes outside the supported set raise ValueError;
there is no torch fallback.  Definition and deviations: INTEGRATION.md §19.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _native
from .grid_encoding import GridLayout
from ._host import _on_device, _prep, _stream

_SUPPORTED = ('supported: decoder.enc containing "hash", "tiled" or "dense" (a grid encoding) whose n_levels * n_features_per_level '
              'is a multiple of 16 up to 64, 2 <= decoder.num_layers <= 8, decoder.hidden_dim 32, 64 or 128, decoder.final_dim a '
              'multiple of 32 up to 256, scene.bound of shape [3, 2], input_ch 3')
BETAS = (0.9, 0.99)                      # train_decoder.py:51
WEIGHT_DECAY, EPS_WEIGHTS, EPS_TABLE = 1e-6, 1e-8, 1e-15     # train_decoder.py:48-49 (torch.optim.Adam's default eps for the MLP)


def _encoding_config(enc: str, desired_resolution: int) -> dict:
    """models/encoding.py:5-46 (get_encoder) for the grid encodings; the other encodings are not implemented"""
    name = str(enc).lower()
    base, n_levels = 16, 16
    if "dense" in name:
        n_levels = 4
        return {"otype": "Grid", "type": "Dense", "n_levels": n_levels, "n_features_per_level": 2, "base_resolution": base,
                "per_level_scale": float(np.exp2(np.log2(desired_resolution / base) / (n_levels - 1))), "interpolation": "Linear"}
    if "hash" in name or "tiled" in name:
        return {"otype": "HashGrid", "n_levels": n_levels, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": base,
                "per_level_scale": float(np.exp2(np.log2(desired_resolution / base) / (n_levels - 1)))}
    raise ValueError(f"FeatureDecoder: decoder.enc {enc!r} is not a grid encoding; {_SUPPORTED}")


class DecoderLayout:
    """Host description of one decoder: the grid's level table, the bounding box and the layer widths (touches no device)."""

    def __init__(self, grid: GridLayout, bound, dims):
        b = np.asarray(bound, dtype=np.float64)
        if b.shape != (3, 2) or grid.n_input_dims != 3:
            raise ValueError(f"FeatureDecoder: scene.bound of shape {list(b.shape)}, input_ch {grid.n_input_dims}; {_SUPPORTED}")
        dims = [int(v) for v in dims]
        if not 2 <= len(dims) - 1 <= _native.DECODER_MAX_LAYERS:
            raise ValueError(f"FeatureDecoder: {len(dims) - 1} layers; {_SUPPORTED}")
        lay = _native.DecoderLayout()
        lay.grid = grid.native
        for k in range(3):
            lay.bound[k][0], lay.bound[k][1] = float(b[k, 0]), float(b[k, 1])
        lay.n_layers = len(dims) - 1
        for i, v in enumerate(dims):
            lay.dims[i] = v
        self.native = lay
        self.grid = grid
        self.dims = dims
        self.n_layers = len(dims) - 1
        self.bound = b
        self.workspace_bytes(1)      # validates the shapes on the host

    @property
    def weight_shapes(self):
        return [(self.dims[l + 1], self.dims[l]) for l in range(self.n_layers)]

    @property
    def n_weights(self) -> int:
        return sum(o * k for o, k in self.weight_shapes)

    def workspace_bytes(self, N: int):
        """(backward workspace bytes, activation record bytes) for N points"""
        ws, act = C.c_size_t(0), C.c_size_t(0)
        st = _native.load().splatraster_decoder_workspace_bytes(C.byref(self.native), int(N), C.byref(ws), C.byref(act))
        if st != _native.OK:
            raise ValueError(f"FeatureDecoder: unsupported shape, layer widths {self.dims}; {_SUPPORTED}")
        return int(ws.value), int(act.value)

    def activation_buffer(self, N: int, device) -> torch.Tensor:
        return torch.empty((max(self.workspace_bytes(N)[1] // 4, 4),), dtype=torch.float32, device=device)

    def split_activations(self, acts: torch.Tensor, N: int) -> dict:
        """views into the activation record of a training forward: `inputs[l]` is the input of layer l (the encoded features,
        then the post-ReLU hidden activations), `f` the unnormalised output, `norm` its length, `xn` the normalised points"""
        off, inputs = 0, []
        for l in range(self.n_layers):
            inputs.append(acts[off:off + N * self.dims[l]].view(N, self.dims[l]))
            off += N * self.dims[l]
        O = self.dims[-1]
        return {"inputs": inputs, "f": acts[off:off + N * O].view(N, O), "norm": acts[off + N * O:off + N * O + N],
                "xn": acts[off + N * O + N:off + N * O + N + 3 * N].view(N, 3)}


def _points(pos: torch.Tensor, dev: torch.device):
    """the points as the kernels read them: contiguous [N, 3] f64 or f32 on `dev` (a CPU f64 tensor is uploaded as f64, so the
    normalisation sees the values the reference's CPU arithmetic sees)"""
    if not torch.is_tensor(pos):
        pos = torch.as_tensor(pos)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"FeatureDecoder: points must be [N, 3], got {list(pos.shape)}")
    if not pos.is_floating_point():
        raise TypeError(f"FeatureDecoder: points must be a float tensor, got {pos.dtype}")
    if pos.is_cuda and pos.device != dev:
        raise RuntimeError(f"FeatureDecoder: points on {pos.device}, parameters on {dev}")
    if pos.requires_grad and torch.is_grad_enabled():
        raise ValueError("FeatureDecoder: a gradient with respect to the points is not implemented (SplatLoc never asks for "
                         "one); pass points that do not require grad, or call splatraster_decoder_backward with dL_dx")
    pos = pos.detach()
    if pos.dtype not in (torch.float32, torch.float64):
        pos = pos.to(torch.float32)
    return pos.to(dev).contiguous()


def _pointer_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _launch_forward(layout: DecoderLayout, x, table, weights, acts):
    dev = table.device
    N = int(x.shape[0])
    out = torch.empty((N, layout.dims[-1]), dtype=torch.float32, device=dev)
    if N > 0:
        with _on_device(dev):
            _native.check(_native.load().splatraster_decoder_forward(
                C.byref(layout.native), N, C.c_void_p(x.data_ptr()), int(x.dtype == torch.float64), C.c_void_p(table.data_ptr()),
                _pointer_array(weights), C.c_void_p(out.data_ptr()), None if acts is None else C.c_void_p(acts.data_ptr()),
                _stream(dev)), "decoder_forward")
    return out


def _launch_backward(layout: DecoderLayout, N, table, weights, acts, g, targets, loss, dw, dtable, workspace):
    dev = table.device
    with _on_device(dev):
        _native.check(_native.load().splatraster_decoder_backward(
            C.byref(layout.native), N, C.c_void_p(table.data_ptr()), _pointer_array(weights), C.c_void_p(acts.data_ptr()),
            None if g is None else C.c_void_p(g.data_ptr()), None if targets is None else C.c_void_p(targets.data_ptr()),
            None if loss is None else C.c_void_p(loss.data_ptr()), C.c_void_p(dw.data_ptr()),
            None if dtable is None else C.c_void_p(dtable.data_ptr()), None, C.c_void_p(workspace.data_ptr()), _stream(dev)),
            "decoder_backward")


class _DecoderFunction(torch.autograd.Function):
    """out = decoder(x); gradients for the table and the weights (never for the points: SplatLoc does not ask for them)"""

    @staticmethod
    def forward(ctx, x, layout, table, *weights):
        dev = table.device
        N = int(x.shape[0])
        ws = [_prep(w, dev) for w in weights]
        tb = _prep(table, dev)
        acts = layout.activation_buffer(N, dev)
        out = _launch_forward(layout, x, tb, ws, acts)
        ctx.layout, ctx.N, ctx.acts = layout, N, acts
        ctx.save_for_backward(table, *weights)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        table, *weights = ctx.saved_tensors
        layout, N, dev = ctx.layout, ctx.N, table.device
        want_t = ctx.needs_input_grad[2]
        dw = torch.zeros((layout.n_weights,), dtype=torch.float32, device=dev)
        dt = torch.zeros_like(table, dtype=torch.float32) if want_t else None
        if N > 0:
            ws_bytes, _ = layout.workspace_bytes(N)
            workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            _launch_backward(layout, N, _prep(table, dev), [_prep(w, dev) for w in weights], ctx.acts, _prep(g, dev), None, None, dw,
                             dt, workspace)
        grads, off = [], 0
        for (o, k), need in zip(layout.weight_shapes, ctx.needs_input_grad[3:]):
            grads.append(dw[off:off + o * k].view(o, k) if need else None)
            off += o * k
        return (None, None, dt, *grads)


class FeatureNet(torch.nn.Module):
    """the parameter container of the reference's FeatureNet: `model` = Sequential(Linear, ReLU, ..., Linear), all bias-free"""

    def __init__(self, input_ch: int, hidden_dim: int, num_layers: int, final_dim: int):
        super().__init__()
        net = []
        for l in range(num_layers):
            net.append(torch.nn.Linear(input_ch if l == 0 else hidden_dim, final_dim if l == num_layers - 1 else hidden_dim,
                                       bias=False))
            if l != num_layers - 1:
                net.append(torch.nn.ReLU(inplace=True))
        self.model = torch.nn.Sequential(*net)

    def weights(self) -> List[torch.nn.Parameter]:
        return [m.weight for m in self.model if isinstance(m, torch.nn.Linear)]


class _Table(torch.nn.Module):
    """`encoding.params` of the reference's tcnn.Encoding: uniform(-1e-4, 1e-4) from a CPU generator seeded 1337, exactly as
    splatloc_amd.grid_encoding.Encoding initialises its own"""

    def __init__(self, layout: GridLayout, seed: int = 1337):
        super().__init__()
        self.layout = layout
        self.n_input_dims, self.n_output_dims = layout.n_input_dims, layout.n_output_dims
        gen = torch.Generator().manual_seed(int(seed))
        init = torch.rand((layout.n_params,), generator=gen, dtype=torch.float32).mul_(2e-4).sub_(1e-4)
        self.params = torch.nn.Parameter(init)


class FeatureDecoder(torch.nn.Module):
    """`FeatureDecoder(config, input_ch=3)` of models/decoders.py.  The table lives on the current ROCm device from construction
    (as tcnn.Encoding's does); the MLP weights move with `.cuda()` as the reference's do."""

    def __init__(self, config, input_ch: int = 3):
        super().__init__()
        self.config = config
        bound = np.array(config["scene"]["bound"])
        if bound.shape != (3, 2) or int(input_ch) != 3:
            raise ValueError(f"FeatureDecoder: scene.bound of shape {list(bound.shape)}, input_ch {input_ch}; {_SUPPORTED}")
        self.bounding_box = torch.from_numpy(bound)
        dim_max = (self.bounding_box[:, 1] - self.bounding_box[:, 0]).max()
        self.resolution_sdf = int(dim_max / config["scene"]["voxel_sdf"])
        dec = config["decoder"]
        enc_cfg = _encoding_config(dec["enc"], self.resolution_sdf)
        hidden, layers, final = int(dec["hidden_dim"]), int(dec["num_layers"]), int(dec["final_dim"])
        grid = GridLayout(3, enc_cfg)
        self.embed_dim = grid.n_output_dims
        if (self.embed_dim % 16 or self.embed_dim > 64 or not 2 <= layers <= 8 or hidden not in (32, 64, 128) or final % 32
                or not 32 <= final <= 256):
            raise ValueError(f"FeatureDecoder: encoded width {self.embed_dim}, hidden_dim {hidden}, num_layers {layers}, "
                             f"final_dim {final}; {_SUPPORTED}")
        self.layout = DecoderLayout(grid, bound, [self.embed_dim] + [hidden] * (layers - 1) + [final])
        self.encoding = _Table(grid)
        self.feature_net = FeatureNet(self.embed_dim, hidden, layers, final)
        if torch.cuda.is_available():
            self.encoding.cuda()

    def _device(self) -> torch.device:
        dev = self.encoding.params.device
        if not dev.type == "cuda":
            raise RuntimeError("FeatureDecoder needs a ROCm device (the HIP kernels are the only implementation)")
        for w in self.feature_net.weights():
            if w.device != dev:
                raise RuntimeError(f"FeatureDecoder: feature_net on {w.device}, encoding on {dev}: call .cuda() as the reference does")
            if w.dtype != torch.float32:
                raise ValueError(f"FeatureDecoder: weights of dtype {w.dtype}; only float32 is implemented")
        return dev

    def forward(self, pos):
        dev = self._device()
        x = _points(pos, dev)
        table, weights = self.encoding.params, self.feature_net.weights()
        if torch.is_grad_enabled() and (table.requires_grad or any(w.requires_grad for w in weights)):
            return _DecoderFunction.apply(x, self.layout, table, *weights)
        return _launch_forward(self.layout, x, _prep(table, dev), [_prep(w, dev) for w in weights], None)


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def cos_loss(network_output, gt):
    sim = torch.cosine_similarity(network_output, gt, dim=1)
    return 1 - sim.mean()


def cos_loss_and_gradients(decoder: "FeatureDecoder", points, features):
    """(loss, [dL/dW_l], dL/dtable, out) of cos_loss(decoder(points), features) in one fused forward + backward, without autograd:
    the route DecoderTrainer.step takes, with the gradients returned instead of applied"""
    dev = decoder._device()
    lay = decoder.layout
    x = _points(points, dev)
    N = int(x.shape[0])
    tgt = _prep(features, dev)
    if N == 0 or tgt is None or tuple(tgt.shape) != (N, lay.dims[-1]):
        raise ValueError(f"cos_loss_and_gradients: points [{N}, 3] need features [{N}, {lay.dims[-1]}] and N >= 1")
    table = _prep(decoder.encoding.params, dev)
    ws = [_prep(w, dev) for w in decoder.feature_net.weights()]
    acts = lay.activation_buffer(N, dev)
    workspace = torch.empty((lay.workspace_bytes(N)[0],), dtype=torch.uint8, device=dev)
    out = _launch_forward(lay, x, table, ws, acts)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    dw = torch.empty((lay.n_weights,), dtype=torch.float32, device=dev)
    dt = torch.zeros_like(table)
    _launch_backward(lay, N, table, ws, acts, None, tgt, loss, dw, dt, workspace)
    grads, off = [], 0
    for o, k in lay.weight_shapes:
        grads.append(dw[off:off + o * k].view(o, k))
        off += o * k
    return loss[0], grads, dt, out


class DecoderTrainer:
    """train_decoder.py:48-51,69-77 as one fused step: forward, cosine loss, backward and Adam over both groups (MLP weights:
    weight_decay 1e-6, eps 1e-8; table: eps 1e-15; betas (0.9, 0.99)).  The optimiser state lives in device tensors; the gradient
    buffers are zeroed by the Adam pass that reads them."""

    def __init__(self, decoder: FeatureDecoder, lr: float = 1e-3):
        self.decoder = decoder
        self.lr = float(lr)
        self.steps = 0
        dev = decoder._device()
        lay = decoder.layout
        self.table = decoder.encoding.params
        self.weights = decoder.feature_net.weights()
        for p in [self.table] + self.weights:
            if not p.is_contiguous() or p.data_ptr() & 15:
                raise ValueError("DecoderTrainer: parameters must be contiguous and 16-byte aligned")
        z = lambda n: torch.zeros((n,), dtype=torch.float32, device=dev)  # noqa: E731
        self.w_grad, self.w_m, self.w_v = z(lay.n_weights), z(lay.n_weights), z(lay.n_weights)
        self.t_grad, self.t_m, self.t_v = (torch.zeros_like(self.table.data) for _ in range(3))
        self._buffers = {}
        self._ptrs = [p.data_ptr() for p in [self.table] + self.weights]

    def _scratch(self, N: int):
        if N not in self._buffers:
            ws, act = self.decoder.layout.workspace_bytes(N)
            dev = self.table.device
            self._buffers[N] = (torch.empty((ws,), dtype=torch.uint8, device=dev),
                                torch.empty((act // 4,), dtype=torch.float32, device=dev))
        return self._buffers[N]

    def step(self, points, features) -> torch.Tensor:
        """one optimisation step on a batch; returns the batch's cosine loss as a device scalar"""
        dev = self.table.device
        lay = self.decoder.layout
        if self.decoder.encoding.params is not self.table or any(a is not b for a, b in
                                                                  zip(self.decoder.feature_net.weights(), self.weights)) \
                or [p.data_ptr() for p in [self.table] + self.weights] != self._ptrs:
            raise RuntimeError("DecoderTrainer: the decoder's parameters were replaced or moved after the trainer was built; "
                               "build a new DecoderTrainer")
        x = _points(points, dev)
        N = int(x.shape[0])
        tgt = _prep(features, dev)
        if N == 0 or tgt is None or tuple(tgt.shape) != (N, lay.dims[-1]):
            raise ValueError(f"DecoderTrainer.step: points [{N}, 3] need features [{N}, {lay.dims[-1]}] and N >= 1")
        workspace, acts = self._scratch(N)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        ws = [w.data for w in self.weights]
        _launch_forward(lay, x, self.table.data, ws, acts)
        _launch_backward(lay, N, self.table.data, ws, acts, None, tgt, loss, self.w_grad, self.t_grad, workspace)
        self.steps += 1
        with _on_device(dev):
            _native.check(_native.load().splatraster_decoder_adam(
                C.byref(lay.native), _pointer_array(ws), C.c_void_p(self.w_grad.data_ptr()), C.c_void_p(self.w_m.data_ptr()),
                C.c_void_p(self.w_v.data_ptr()), C.c_void_p(self.table.data_ptr()), C.c_void_p(self.t_grad.data_ptr()),
                C.c_void_p(self.t_m.data_ptr()), C.c_void_p(self.t_v.data_ptr()), self.steps, self.lr, self.lr, BETAS[0], BETAS[1],
                EPS_WEIGHTS, EPS_TABLE, WEIGHT_DECAY, _stream(dev)), "decoder_adam")
        return loss[0]

    def state_dict(self) -> dict:
        """the state in the form of train_decoder.py's torch.optim.Adam: group 0 = the MLP weights, group 1 = the table"""
        state, off = {}, 0
        step = torch.tensor(float(self.steps))
        for i, (o, k) in enumerate(self.decoder.layout.weight_shapes):
            state[i] = {"step": step.clone(), "exp_avg": self.w_m[off:off + o * k].view(o, k).clone(),
                        "exp_avg_sq": self.w_v[off:off + o * k].view(o, k).clone()}
            off += o * k
        n = len(self.weights)
        state[n] = {"step": step.clone(), "exp_avg": self.t_m.clone(), "exp_avg_sq": self.t_v.clone()}
        common = {"lr": self.lr, "betas": BETAS, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                  "differentiable": False, "fused": None}
        groups = [dict(common, weight_decay=WEIGHT_DECAY, eps=EPS_WEIGHTS, params=list(range(n))),
                  dict(common, weight_decay=0, eps=EPS_TABLE, params=[n])]
        return {"state": state if self.steps else {}, "param_groups": groups}


def train_decoder(decoder: FeatureDecoder, points, features, num_epochs: int = 41, batch_size: int = 256, lr: float = 1e-3,
                  seed: int = 0, permutations: Optional[list] = None) -> torch.Tensor:
    """The loop of train_decoder.py:64-82 (shuffle=True, drop_last=False): the data is uploaded once, every epoch walks a
    permutation (from a CPU generator seeded `seed`, or `permutations[epoch]`) in batches of `batch_size`, the short last batch as
    its own step.  Returns the per-step losses as one device tensor."""
    trainer = DecoderTrainer(decoder, lr=lr)
    dev = trainer.table.device
    pts = _points(points, dev)
    feats = _prep(features, dev)
    n = int(pts.shape[0])
    if feats is None or feats.shape[0] != n or n == 0:
        raise ValueError("train_decoder: points [n, 3] and features [n, final_dim] with n >= 1")
    gen = torch.Generator().manual_seed(int(seed))
    losses = []
    for epoch in range(int(num_epochs)):
        perm = torch.randperm(n, generator=gen) if permutations is None else torch.as_tensor(permutations[epoch]).long()
        perm = perm.to(dev)
        for start in range(0, int(perm.shape[0]), int(batch_size)):
            sel = perm[start:start + int(batch_size)]
            losses.append(trainer.step(pts[sel], feats[sel]))
    return torch.stack(losses) if losses else torch.zeros((0,), dtype=torch.float32, device=dev)
