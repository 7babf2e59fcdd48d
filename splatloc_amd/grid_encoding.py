"""tinycudann.Encoding replacement for the grid encodings of FeatureDecoder (models/encoding.py:3,33-46).

The encoding itself is the HIP of csrc/grid_encoding.hip behind the C ABI (include/splatraster.h); the level table is laid out
once on the host (splatraster_grid_encoding_layout).  Only the multiresolution grids with linear interpolation in fp32 exist
here: every other tiny-cuda-nn encoding, interpolation or precision raises ValueError, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import torch

from . import _native
from ._host import _on_device, _prep, _stream

_GRID_OTYPES = {"hashgrid": _native.GRID_HASH, "densegrid": _native.GRID_DENSE, "tiledgrid": _native.GRID_TILED}
_GRID_TYPES = {"hash": _native.GRID_HASH, "dense": _native.GRID_DENSE, "tiled": _native.GRID_TILED}
_SUPPORTED = ('supported: otype "HashGrid", "DenseGrid", "TiledGrid" or "Grid" with type "Hash" / "Dense" / "Tiled", '
              'interpolation "Linear", n_input_dims 2 or 3, n_features_per_level 1, 2, 4 or 8, 1 <= n_levels <= 32, '
              '1 <= log2_hashmap_size <= 30, dtype torch.float32')


class GridLayout:
    """The level table of one grid-encoding configuration (host only: computing it touches no device)."""

    def __init__(self, n_input_dims: int, encoding_config: dict):
        cfg = dict(encoding_config)
        otype = str(cfg.get("otype", "")).lower()
        if otype == "grid":
            gtype = _GRID_TYPES.get(str(cfg.get("type", "Hash")).lower())
        else:
            gtype = _GRID_OTYPES.get(otype)
        if gtype is None:
            raise ValueError(f"tinycudann.Encoding: unsupported encoding {encoding_config!r}; {_SUPPORTED}")
        interp = str(cfg.get("interpolation", "Linear")).lower()
        if interp != "linear":
            raise ValueError(f"tinycudann.Encoding: unsupported interpolation {cfg['interpolation']!r}; {_SUPPORTED}")
        try:
            D = int(n_input_dims)
            L = int(cfg.get("n_levels", 16))
            F = int(cfg.get("n_features_per_level", 2))
            log2_T = int(cfg.get("log2_hashmap_size", 19))
            base = int(cfg.get("base_resolution", 16))
            pls = float(cfg.get("per_level_scale", 2.0))
        except (TypeError, ValueError) as e:
            raise ValueError(f"tinycudann.Encoding: malformed configuration {encoding_config!r} ({e}); {_SUPPORTED}") from e
        lay = _native.GridLayout()
        st = _native.load().splatraster_grid_encoding_layout(D, L, F, log2_T, base, pls, gtype, C.byref(lay))
        if st != _native.OK:
            raise ValueError(f"tinycudann.Encoding: unsupported configuration n_input_dims={D} {encoding_config!r}; "
                             f"{_SUPPORTED} (base_resolution >= 1, per_level_scale > 0, at most 2^31 table entries)")
        self.native = lay
        self.grid_type = gtype
        self.n_input_dims = D
        self.n_levels = L
        self.n_features_per_level = F
        self.n_output_dims = L * F
        self.n_params = int(lay.n_params)

    @property
    def offsets(self):
        return [int(v) for v in self.native.offset[:self.n_levels]]

    @property
    def sizes(self):
        return [int(v) for v in self.native.size[:self.n_levels]]

    @property
    def resolutions(self):
        return [int(v) for v in self.native.resolution[:self.n_levels]]

    @property
    def scales(self):
        return [float(v) for v in self.native.scale[:self.n_levels]]


class _GridEncodingFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, params: torch.Tensor, layout: GridLayout) -> torch.Tensor:
        dev = params.device
        N = int(x.shape[0])
        if params.numel() != layout.n_params:       # the kernels index the whole table
            raise ValueError(f"tinycudann.Encoding: params has {params.numel()} entries, the layout needs {layout.n_params}")
        out = torch.empty((N, layout.n_output_dims), dtype=torch.float32, device=dev)
        xs = _prep(x, dev)
        ps = _prep(params, dev)
        if N > 0:
            with _on_device(dev):
                _native.check(_native.load().splatraster_grid_encoding_forward(
                    C.byref(layout.native), N, C.c_void_p(xs.data_ptr()), C.c_void_p(ps.data_ptr()),
                    C.c_void_p(out.data_ptr()), _stream(dev)), "grid_encoding_forward")
        ctx.layout = layout
        ctx.save_for_backward(x, params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g: torch.Tensor):
        x, params = ctx.saved_tensors
        layout = ctx.layout
        dev = params.device
        N = int(x.shape[0])
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty((N, layout.n_input_dims), dtype=torch.float32, device=dev) if want_x else None
        dp = torch.zeros((layout.n_params,), dtype=torch.float32, device=dev) if want_p else None
        if tuple(g.shape) != (N, layout.n_output_dims):
            raise ValueError(f"tinycudann.Encoding: gradient of shape {list(g.shape)}, expected [{N}, {layout.n_output_dims}]")
        if N > 0 and (want_x or want_p):
            xs, ps, gs = _prep(x, dev), _prep(params, dev), _prep(g, dev)
            with _on_device(dev):
                _native.check(_native.load().splatraster_grid_encoding_backward(
                    C.byref(layout.native), N, C.c_void_p(xs.data_ptr()), C.c_void_p(ps.data_ptr()),
                    C.c_void_p(gs.data_ptr()), None if dp is None else C.c_void_p(dp.data_ptr()),
                    None if dx is None else C.c_void_p(dx.data_ptr()), _stream(dev)), "grid_encoding_backward")
        return dx, dp, None


class Encoding(torch.nn.Module):
    """`tcnn.Encoding(n_input_dims, encoding_config, seed=1337, dtype=torch.float)` for the grid encodings.

    Owns one parameter, `params` [n_params] f32 on the current ROCm device, initialised uniform(-1e-4, 1e-4) from a torch
    generator seeded with `seed`.  `dtype=None` means float32 (the only precision implemented; tiny-cuda-nn would pick its
    build's default there)."""

    def __init__(self, n_input_dims: int, encoding_config: dict, seed: int = 1337, dtype: Optional[torch.dtype] = None):
        super().__init__()
        if dtype is not None and dtype != torch.float32:
            raise ValueError(f"tinycudann.Encoding: dtype {dtype} is not implemented; {_SUPPORTED}")
        self.layout = GridLayout(n_input_dims, encoding_config)
        self.n_input_dims = self.layout.n_input_dims
        self.n_output_dims = self.layout.n_output_dims
        self.encoding_config = encoding_config
        self.seed = seed
        self.dtype = torch.float32
        if not torch.cuda.is_available():
            raise RuntimeError("tinycudann.Encoding needs a ROCm device (the HIP kernels are the only implementation)")
        gen = torch.Generator().manual_seed(int(seed))
        init = torch.rand((self.layout.n_params,), generator=gen, dtype=torch.float32).mul_(2e-4).sub_(1e-4)
        self.params = torch.nn.Parameter(init.to(torch.device("cuda", torch.cuda.current_device())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dev = self.params.device
        if not x.is_cuda:
            warnings.warn("tinycudann.Encoding: input is not on a ROCm device; it is copied to "
                          f"{dev} (suboptimal performance)", stacklevel=2)
            x = x.to(dev)
        elif x.device != dev:
            raise RuntimeError(f"tinycudann.Encoding: input on {x.device}, parameters on {dev}")
        if not x.is_floating_point():
            raise TypeError(f"tinycudann.Encoding: input must be a float tensor, got {x.dtype}")
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError(f"tinycudann.Encoding: input must be [N, {self.n_input_dims}], got {list(x.shape)}")
        x = x.to(torch.float32).contiguous()
        return _GridEncodingFunction.apply(x, self.params, self.layout)

    def extra_repr(self) -> str:
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, encoding_config={self.encoding_config}"
