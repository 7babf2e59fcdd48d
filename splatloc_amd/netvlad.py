"""The NetVLAD head on the device: everything behind the network's convolution stack.

`features` [B,D,h,w] (or [B,D,N]), the backbone's map, goes in; the global descriptor `localize.retrieve` and
`localize.generate_retrieval_file` take comes out: per-location normalisation, the soft assignment to K clusters, the residual
aggregation into a D x K matrix, intra-normalisation, the descriptor's normalisation, the whitening projection and a last
normalisation.  hloc's NetVLAD layer is not part of the reference tree; include/splatraster.h (splatraster_netvlad_*) and
INTEGRATION.md §25 hold the definitions this module implements, which are this project's own.

Everything is the HIP of csrc/netvlad_head.hip behind the C ABI, on the current stream, without a host synchronisation and without
float atomics: a row of the batch is bit-identical whatever the batch size.  Inputs are float32 contiguous device tensors; anything
else raises before device work.  There is no CPU fallback and no torch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native
from ._host import _stream, device, ptr, workspace

MAX_K = 64          # SPLATRASTER_NETVLAD_MAX_K
INTRANORM = 1       # SPLATRASTER_NETVLAD_INTRANORM
L2NORM = 2          # SPLATRASTER_NETVLAD_L2NORM


def _check(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}; the NetVLAD head runs on a ROCm device only (there is no CPU fallback)")
    if t.dtype is not torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach()


def tiles() -> dict:
    """The tile constants of the launch geometry (host only): `n_step` locations per assign workgroup and aggregation step, `d_tile`
    d rows per aggregation workgroup, `i_slice` columns per projection workgroup, `o_tile` x `b_tile` weight rows x images of a
    projection tile."""
    v = [C.c_int32(0) for _ in range(5)]
    _native.check(_native.load().splatraster_netvlad_tiles(*(C.byref(x) for x in v)), "splatraster_netvlad_tiles")
    return dict(zip(("n_step", "d_tile", "i_slice", "o_tile", "b_tile"), (int(x.value) for x in v)))


class NetVLADHead:
    """score_weight [K,D] (or [K,D,1], the 1x1 convolution's own shape), centers [D,K], optional score_bias [K], optional whitening
    whiten_weight [O,D K] and whiten_bias [O]: float32 contiguous tensors on one ROCm device.  intranorm: normalise every cluster's
    residual column before the descriptor is flattened."""

    def __init__(self, score_weight, centers, score_bias=None, whiten_weight=None, whiten_bias=None, intranorm=True):
        w = _check(score_weight, "score_weight")
        if w.dim() == 3 and w.shape[2] == 1:
            w = w[:, :, 0]
        c = _check(centers, "centers")
        if w.dim() != 2 or c.dim() != 2 or min(w.shape) < 1 or tuple(c.shape) != (w.shape[1], w.shape[0]):
            raise ValueError(f"score_weight must be [K, D] and centers [D, K], got {tuple(score_weight.shape)} and {tuple(centers.shape)}")
        self.K, self.D = int(w.shape[0]), int(w.shape[1])
        if self.K > MAX_K:
            raise ValueError(f"K = {self.K} clusters: at most {MAX_K} are supported")
        if self.D * self.K >= 1 << 31:
            raise ValueError(f"D K = {self.D * self.K}: fewer than 2^31 descriptor entries are supported")
        self.device = w.device
        self.score_weight, self.centers = w, c
        self.score_bias = self._param(score_bias, "score_bias", (self.K,))
        self.O = 0
        self.whiten_weight = self.whiten_bias = None
        if whiten_weight is not None:
            ww = _check(whiten_weight, "whiten_weight")
            if ww.dim() != 2 or ww.shape[0] < 1 or ww.shape[1] != self.D * self.K:
                raise ValueError(f"whiten_weight must be [O, {self.D * self.K}], got {tuple(ww.shape)}")
            self.whiten_weight = self._param(ww, "whiten_weight", tuple(ww.shape))
            self.O = int(ww.shape[0])
            self.whiten_bias = self._param(whiten_bias, "whiten_bias", (self.O,))
        elif whiten_bias is not None:
            raise ValueError("whiten_bias without whiten_weight")
        if c.device != self.device:
            raise ValueError("the head's tensors must be on one device")
        self.intranorm = bool(intranorm)
        self._ws: dict = {}

    def _param(self, t, name, shape):
        if t is None:
            return None
        t = _check(t, name)
        if tuple(t.shape) != shape or t.device != self.device:
            raise ValueError(f"{name} must be {list(shape)} on {self.device}, got {tuple(t.shape)} on {t.device}")
        return t

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "", intranorm: bool = True):
        """The head of a state dict with this project's names for an hloc-style checkpoint: `netvlad.score_proj.weight` ([K,D] or
        [K,D,1]), optional `netvlad.score_proj.bias`, `netvlad.centers` [D,K], optional `whiten.weight` and `whiten.bias`.  The tensors
        are moved to the current device as float32."""
        dev = device("the NetVLAD head")

        def get(name, required=False):
            t = sd.get(prefix + name)
            if t is None:
                if required:
                    raise KeyError(f"{prefix + name} is missing from the state dict")
                return None
            return t.detach().to(device=dev, dtype=torch.float32).contiguous()

        return cls(get("netvlad.score_proj.weight", True), get("netvlad.centers", True), get("netvlad.score_proj.bias"),
                   get("whiten.weight"), get("whiten.bias"), intranorm)

    # ---- plumbing ----------------------------------------------------------------------------------------------------------------

    def _features(self, features) -> torch.Tensor:
        f = _check(features, "features")
        if f.dim() == 4:
            f = f.reshape(f.shape[0], f.shape[1], -1)
        if f.dim() != 3 or f.shape[1] != self.D or f.shape[2] < 1:
            raise ValueError(f"features must be [B, {self.D}, h, w] or [B, {self.D}, N], got {tuple(features.shape)}")
        if f.device != self.device:
            raise ValueError(f"features are on {f.device}, the head on {self.device}")
        return f

    def _workspace(self, b: int, n: int) -> torch.Tensor:
        key = (b, n)
        ws = self._ws.get(key)
        if ws is None:
            nb = C.c_size_t(0)
            _native.check(_native.load().splatraster_netvlad_workspace_size(b, self.D, self.K, n, max(self.O, 1), C.byref(nb)),
                          "splatraster_netvlad_workspace_size")
            ws = self._ws[key] = workspace(nb.value, self.device)
        return ws

    def _assign(self, f, ws):
        b, _, n = (int(s) for s in f.shape)
        a = torch.empty((b, self.K, n), dtype=torch.float32, device=self.device)
        inv = torch.empty((b, n), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = _native.load().splatraster_netvlad_assign(b, self.D, self.K, n, ptr(f), ptr(self.score_weight), ptr(self.score_bias),
                                                           ptr(a), ptr(inv), ptr(ws), ws.numel(), _stream(self.device))
        _native.check(st, "splatraster_netvlad_assign")
        return a, inv

    def _aggregate(self, f, a, inv, flags, ws):
        b, _, n = (int(s) for s in f.shape)
        v = torch.empty((b, self.D * self.K), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = _native.load().splatraster_netvlad_aggregate(b, self.D, self.K, n, ptr(f), ptr(a), ptr(inv), ptr(self.centers), flags,
                                                              ptr(v), ptr(ws), ws.numel(), _stream(self.device))
        _native.check(st, "splatraster_netvlad_aggregate")
        return v

    def _project(self, v, ws):
        b = int(v.shape[0])
        y = torch.empty((b, self.O), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = _native.load().splatraster_netvlad_project(b, self.O, self.D * self.K, ptr(v), ptr(self.whiten_weight),
                                                            ptr(self.whiten_bias), L2NORM, ptr(y), ptr(ws), ws.numel(),
                                                            _stream(self.device))
        _native.check(st, "splatraster_netvlad_project")
        return y

    def _flags(self, raw: bool) -> int:
        return 0 if raw else (INTRANORM if self.intranorm else 0) | L2NORM

    # ---- the stages --------------------------------------------------------------------------------------------------------------

    def assign(self, features):
        """(assign [B,K,N], inv_norm [B,N]): the soft assignment of every location and the reciprocal of its descriptor's norm."""
        f = self._features(features)
        return self._assign(f, self._workspace(int(f.shape[0]), int(f.shape[2])))

    def vlad(self, features, raw: bool = False):
        """v [B, D K], flattened as d * K + k: the aggregated residuals, intra-normalised (when the head is) and of unit length; raw:
        the residual matrix itself."""
        f = self._features(features)
        ws = self._workspace(int(f.shape[0]), int(f.shape[2]))
        a, inv = self._assign(f, ws)
        return self._aggregate(f, a, inv, self._flags(raw), ws)

    def project(self, v):
        """y [B,O]: the whitening of v [B, D K], of unit length."""
        if self.whiten_weight is None:
            raise ValueError("this head has no whitening projection")
        v = _check(v, "v")
        if v.dim() != 2 or v.shape[1] != self.D * self.K or v.device != self.device:
            raise ValueError(f"v must be [B, {self.D * self.K}] on {self.device}, got {tuple(v.shape)} on {v.device}")
        return self._project(v, self._workspace(int(v.shape[0]), 1))

    def __call__(self, features):
        """The global descriptors [B,O] of a batch of maps ([B, D K] for a head without whitening), unit rows: `assign`, `vlad` and
        `project` as one launch sequence on one workspace, bit-identical to the staged calls."""
        f = self._features(features)
        ws = self._workspace(int(f.shape[0]), int(f.shape[2]))
        a, inv = self._assign(f, ws)
        v = self._aggregate(f, a, inv, self._flags(False), ws)
        return v if self.whiten_weight is None else self._project(v, ws)
