"""The convolution backbones on the device: SuperPoint's encoder with its two heads, and NetVLAD's VGG16 trunk.

Both networks are one layer repeated: a 3x3 convolution with zero padding 1, bias and ReLU, sometimes followed by a 2x2 / stride-2
max pool, and a 1x1 convolution at the end of SuperPoint's heads.  `conv2d` is that layer (csrc/conv2d.hip: an implicit GEMM on the
exact-f32 MFMA whose summation order include/splatraster.h writes down); `SuperPointEncoder` and `VGG16Trunk` are the two layer
tables; `SuperPointExtractor` and `NetVLAD` join them with the existing `superpoint` and `netvlad` modules, so an image goes from
pixels to keypoints and descriptors, or to a retrieval row, without a framework convolution.

Neither hloc's SuperPoint nor its NetVLAD is part of the reference tree, and no pretrained weights are: the layer tables below
(MagicLeap's SuperPoint layout, torchvision's VGG16 `features` cut where hloc cuts it) are this project's own contract and parity
with those networks is unpinned.

Everything is HIP behind the C ABI, on the current stream, without a host synchronisation and without float atomics: an image of
the batch is bit-identical whatever the batch size.  Inputs are float32 contiguous device tensors; anything else raises before
device work.  There is no CPU fallback and no torch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native, superpoint
from ._host import _stream, device, ptr
from .netvlad import NetVLADHead

RELU = 1     # SPLATRASTER_CONV_RELU
POOL2 = 2    # SPLATRASTER_CONV_POOL2

# (name, pool after it): the shared encoder; every layer is 3x3 + ReLU
SUPERPOINT_ENCODER = (("conv1a", False), ("conv1b", True), ("conv2a", False), ("conv2b", True), ("conv3a", False), ("conv3b", True),
                      ("conv4a", False), ("conv4b", False))
SUPERPOINT_WIDTHS = {"conv1a": (1, 64), "conv1b": (64, 64), "conv2a": (64, 64), "conv2b": (64, 64), "conv3a": (64, 128),
                     "conv3b": (128, 128), "conv4a": (128, 128), "conv4b": (128, 128), "convPa": (128, 256), "convPb": (256, 65),
                     "convDa": (128, 256), "convDb": (256, 256)}
# torchvision's vgg16().features: index of every convolution, (Cin, Cout), and whether a pool (the index behind its ReLU) follows
VGG16_CONVS = ((0, 3, 64, False), (2, 64, 64, True), (5, 64, 128, False), (7, 128, 128, True), (10, 128, 256, False),
               (12, 256, 256, False), (14, 256, 256, True), (17, 256, 512, False), (19, 512, 512, False), (21, 512, 512, True),
               (24, 512, 512, False), (26, 512, 512, False), (28, 512, 512, False))


def _check(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}; the convolutions run on a ROCm device only (there is no CPU fallback)")
    if t.dtype is not torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach()


def tiles() -> dict:
    """The tile constants of the launch geometry (host only): `co_tile` output channels per workgroup, its `px_rows` x `px_cols` tile
    of output pixels, and `ci_chunk` input channels staged per step (the chunk of the declared chain order)."""
    v = [C.c_int32(0) for _ in range(4)]
    _native.check(_native.load().splatraster_conv2d_tiles(*(C.byref(x) for x in v)), "splatraster_conv2d_tiles")
    return dict(zip(("co_tile", "px_rows", "px_cols", "ci_chunk"), (int(x.value) for x in v)))


def out_size(h: int, w: int, pool: bool):
    return (h // 2, w // 2) if pool else (h, w)


def _check_layer(x, weight, bias, pool):
    """the shapes of one layer; returns (B, Cin, Cout, H, W, ksize)"""
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"x must be [B, Cin, H, W] and weight [Cout, Cin, k, k], got {tuple(x.shape)} and {tuple(weight.shape)}")
    b, cin, h, w = (int(s) for s in x.shape)
    cout, wcin, k, k2 = (int(s) for s in weight.shape)
    if k != k2 or k not in (1, 3):
        raise ValueError(f"the kernel must be 1x1 or 3x3, got {k}x{k2}")
    if wcin != cin or min(cin, cout, h, w) < 1:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} do not make a layer")
    if pool and min(h, w) < 2:
        raise ValueError(f"a {h} x {w} map cannot be pooled")
    if max(cin, cout) * h * w >= 1 << 31:
        raise ValueError(f"a map of {max(cin, cout)} x {h} x {w} elements: fewer than 2^31 per image are supported")
    if weight.device != x.device or (bias is not None and (tuple(bias.shape) != (cout,) or bias.device != x.device)):
        raise ValueError(f"weight and bias [{cout}] must be on {x.device}")
    return b, cin, cout, h, w, k


def _launch(x, weight, bias, flags, out, shape):
    b, cin, cout, h, w, k = shape
    with torch.cuda.device(x.device):
        st = _native.load().splatraster_conv2d(b, cin, cout, h, w, k, ptr(x), ptr(weight), ptr(bias), flags, ptr(out), None, 0,
                                               _stream(x.device))
    _native.check(st, "splatraster_conv2d")


def conv2d(x, weight, bias=None, relu: bool = False, pool: bool = False, out=None) -> torch.Tensor:
    """One layer: the stride-1 cross-correlation of x [B,Cin,H,W] with weight [Cout,Cin,k,k] (k = 1 or 3, zero padding (k - 1) / 2),
    + bias, ReLU, then a 2x2 / stride-2 max pool in floor mode.  Returns [B,Cout,H,W] ([B,Cout,H/2,W/2] pooled); `out` may hold it
    (the first elements of a larger contiguous float32 buffer are used) and must not overlap x."""
    x, weight = _check(x, "x"), _check(weight, "weight")
    bias = None if bias is None else _check(bias, "bias")
    shape = _check_layer(x, weight, bias, pool)
    b, _, cout, h, w, _ = shape
    ho, wo = out_size(h, w, pool)
    n = b * cout * ho * wo
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=x.device)
    else:
        _check(out, "out")
        if out.numel() < n or out.device != x.device:
            raise ValueError(f"out must hold {n} elements on {x.device}")
    res = out.view(-1)[:n].view(b, cout, ho, wo)
    if b:
        _launch(x, weight, bias, (RELU if relu else 0) | (POOL2 if pool else 0), res, shape)
    return res


def preprocess(image, out=None) -> torch.Tensor:
    """NetVLAD's input normalisation of an RGB batch [B,3,H,W] in [0,1]: clamp(image * 255, 0, 255) - (123.68, 116.779, 103.939)."""
    image = _check(image, "image")
    if image.dim() != 4 or image.shape[1] != 3 or min(image.shape[2:]) < 1:
        raise ValueError(f"image must be [B, 3, H, W], got {tuple(image.shape)}")
    b, _, h, w = (int(s) for s in image.shape)
    if 3 * h * w >= 1 << 31:
        raise ValueError(f"an image of 3 x {h} x {w} elements: fewer than 2^31 are supported")
    if out is None:
        out = torch.empty_like(image)
    with torch.cuda.device(image.device):
        st = _native.load().splatraster_netvlad_preprocess(b, h, w, ptr(image), ptr(out), _stream(image.device))
    _native.check(st, "splatraster_netvlad_preprocess")
    return out


def _layer_params(sd, name, cin, cout, k, dev):
    """(weight, bias) of `name` from a state dict, checked against the table and moved to `dev` as float32"""
    w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
    if w is None or b is None:
        raise KeyError(f"{name}.weight / {name}.bias are missing from the state dict")
    if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
        raise ValueError(f"{name}: expected weight {(cout, cin, k, k)} and bias {(cout,)}, got {tuple(w.shape)} and {tuple(b.shape)}")
    return (w.detach().to(device=dev, dtype=torch.float32).contiguous(), b.detach().to(device=dev, dtype=torch.float32).contiguous())


def superpoint_shapes(h: int, w: int) -> list:
    """(name, H, W of the layer's output) down SuperPointEncoder's table for an h x w image; host only"""
    res = []
    for name, pool in SUPERPOINT_ENCODER:
        h, w = out_size(h, w, pool)
        res.append((name, h, w))
    return res + [(n, h, w) for n in ("convPa", "convPb", "convDa", "convDb")]


def vgg16_shapes(h: int, w: int) -> list:
    """(features index, H, W of the layer's output) down VGG16Trunk's table for an h x w image; host only"""
    res = []
    for idx, _, _, pool in VGG16_CONVS:
        h, w = out_size(h, w, pool)
        res.append((idx, h, w))
    return res


class _Net:
    """a layer table's plumbing: the input check and two ping-pong buffers per input shape"""

    def __init__(self, what: str, cin: int, min_size: int):
        self.device = device(what)
        self.what, self.cin, self.min_size = what, cin, min_size
        self._bufs: dict = {}

    def _input(self, image) -> torch.Tensor:
        x = _check(image, "image")
        if x.dim() != 4 or x.shape[1] != self.cin or min(x.shape[2:]) < self.min_size:
            raise ValueError(f"image must be [B, {self.cin}, H, W] with H, W >= {self.min_size}, got {tuple(image.shape)}")
        if x.device != self.device:
            raise ValueError(f"image is on {x.device}, {self.what} on {self.device}")
        return x

    def _buffers(self, key, numel: int):
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = tuple(torch.empty(max(numel, 1), dtype=torch.float32, device=self.device) for _ in range(2))
        return bufs


class SuperPointEncoder(_Net):
    """SuperPoint's shared encoder and both heads, in MagicLeap's / hloc's layout: state-dict keys `conv1a` .. `conv4b`, `convPa`,
    `convPb`, `convDa`, `convDb`, each with `.weight` and `.bias` (an optional `prefix` in front).  Widths 1 -> 64 -> 64 | 64 -> 64 |
    128 -> 128 | 128 -> 128, every layer 3x3 + ReLU, a 2x2 max pool behind the b-layer of blocks 1 to 3; heads 128 -> 256 (3x3, ReLU)
    -> 65 (detector) or 256 (descriptor) by a 1x1 convolution without ReLU.  The definition is this project's own (see the module's
    docstring): parity with a pretrained network is unpinned."""

    def __init__(self, state_dict, prefix: str = ""):
        super().__init__("the SuperPoint encoder", 1, 8)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.params = {n: _layer_params(sd, n, cin, cout, 1 if n in ("convPb", "convDb") else 3, self.device)
                       for n, (cin, cout) in SUPERPOINT_WIDTHS.items()}

    def __call__(self, image, taps: dict = None):
        """image [B,1,H,W] (H, W >= 8; sizes that are no multiple of 8 floor at every pool) -> (semi [B,65,H/8,W/8], coarse
        [B,256,H/8,W/8]), the inputs of `superpoint.detect`: one launch sequence on two ping-pong buffers.  taps: a dict that
        receives a copy of every layer's output by name (tests)."""
        x = self._input(image)
        b, _, h, w = (int(s) for s in x.shape)
        a, c = self._buffers((b, h, w), b * 64 * h * w)
        for name, pool in SUPERPOINT_ENCODER:
            x = conv2d(x, *self.params[name], relu=True, pool=pool, out=a)
            a, c = c, a
            if taps is not None:
                taps[name] = x.clone()
        outs = []
        for first, last in (("convPa", "convPb"), ("convDa", "convDb")):
            mid = conv2d(x, *self.params[first], relu=True, out=a)   # x stays in the other buffer for the second head
            outs.append(conv2d(mid, *self.params[last]))
            if taps is not None:
                taps[first], taps[last] = mid.clone(), outs[-1]
        return outs[0], outs[1]


class SuperPointExtractor:
    """`SuperPointEncoder` joined with the `superpoint` module (NMS, selection, descriptor sampling): an image in, keypoints, scores
    and descriptors out, with the module's own argument names and defaults."""

    def __init__(self, state_dict, nms_radius: int = 4, keypoint_threshold: float = 0.005, max_keypoints: int = 4096,
                 remove_borders: int = 4, prefix: str = ""):
        self.encoder = SuperPointEncoder(state_dict, prefix)
        self.config = dict(nms_radius=nms_radius, keypoint_threshold=keypoint_threshold, max_keypoints=max_keypoints,
                           remove_borders=remove_borders)

    def detect(self, image) -> dict:
        """`superpoint.detect` of the encoder's outputs: padded device tensors, nothing read back"""
        return superpoint.detect(*self.encoder(image), **self.config)

    def postprocess(self, image, original_size=None) -> list:
        """`superpoint.postprocess` of the encoder's outputs: hloc's per-image dicts"""
        return superpoint.postprocess(*self.encoder(image), **self.config, original_size=original_size)

    def dense_descriptors(self, image, rows=None, out=None) -> torch.Tensor:
        """`superpoint.dense_descriptors` of the encoder's descriptor map: [B,rows,8 (W/8),256], what fusion.integrate_frames reads"""
        return superpoint.dense_descriptors(self.encoder(image)[1], rows, out)


class VGG16Trunk(_Net):
    """NetVLAD's backbone: the 13 convolutions of torchvision's `vgg16().features` (state-dict keys `<prefix><index>.weight` /
    `.bias` for index 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), all 3x3, ReLU behind every one but the last, a 2x2 max pool
    behind indices 2, 7, 14 and 21, nothing behind index 28 (hloc slices the Sequential `[:-2]`).  The definition is this project's
    own (see the module's docstring): parity with a pretrained network is unpinned."""

    def __init__(self, state_dict, prefix: str = "backbone."):
        super().__init__("the VGG16 trunk", 3, 16)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.params = {idx: _layer_params(sd, str(idx), cin, cout, 3, self.device) for idx, cin, cout, _ in VGG16_CONVS}

    def __call__(self, image, taps: dict = None):
        """image [B,3,H,W], already normalised (`preprocess`), H, W >= 16 -> [B,512,H/16,W/16]: one launch sequence on two ping-pong
        buffers.  taps: a dict that receives a copy of every layer's output by its index (tests)."""
        x = self._input(image)
        b, _, h, w = (int(s) for s in x.shape)
        a, c = self._buffers((b, h, w), b * 64 * h * w)
        last = VGG16_CONVS[-1][0]
        for idx, _, _, pool in VGG16_CONVS:
            x = conv2d(x, *self.params[idx], relu=idx != last, pool=pool, out=None if idx == last else a)
            a, c = c, a
            if taps is not None:
                taps[idx] = x if idx == last else x.clone()
        return x


class NetVLAD:
    """Pixels to a global descriptor: `preprocess`, `VGG16Trunk` and `NetVLADHead.from_state_dict` of one state dict (the trunk under
    `backbone.`, the head under netvlad.py's names).  The rows feed `localize.retrieve` unchanged."""

    def __init__(self, state_dict, prefix: str = "", intranorm: bool = True):
        self.trunk = VGG16Trunk(state_dict, prefix + "backbone.")
        self.head = NetVLADHead.from_state_dict(state_dict, prefix, intranorm)
        if self.head.D != 512:
            raise ValueError(f"the head takes {self.head.D} channels, the trunk gives 512")

    def __call__(self, image) -> torch.Tensor:
        """image [B,3,H,W] in [0,1] (RGB) -> [B,O] unit rows ([B, D K] for a head without whitening)"""
        x = self.trunk._input(image)
        return self.head(self.trunk(preprocess(x)))
