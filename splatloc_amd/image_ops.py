"""Frame preparation of SplatLoc's key-frame loop and of test.py on the device: the Scharr image gradients and their validity
mask (utils/utils.py:4-38), Camera.compute_grad_mask for both dataset types (utils/camera_utils.py:145-172) and the masked
medians of get_median_depth (utils/utils.py:85-96).

Everything is the HIP of csrc/image_ops.hip behind the C ABI (include/splatraster.h, splatraster_image_gradient,
splatraster_grad_mask, splatraster_masked_median), on the current stream, several frames per launch sequence and without a host
synchronisation.  `image_gradient`, `image_gradient_mask`, `get_median_depth` and `compute_grad_mask` are drop-ins for the
reference's functions of those names; `compute_grad_masks` and `masked_median` are the batched calls.
Inputs are float32 contiguous device tensors; anything else raises before device work.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native
from ._host import _stream, ptr, workspace

REPLICA, GLOBAL = 0, 1   # SPLATRASTER_GRAD_MASK_*
BLOCKS = 32              # the Replica branch's blocks per side
PATHS = {0: "none", 1: "lds_small", 2: "lds_big", 3: "global"}   # splatraster_debug_image_ops_path


def _check(t, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}; image_ops runs on a ROCm device only (there is no CPU fallback)")
    if t.dtype is not dtype:
        raise ValueError(f"{name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach()


def path(H: int, W: int) -> str:
    """which internal path the Replica branch takes for H x W frames (host only)"""
    return PATHS[int(_native.load().splatraster_debug_image_ops_path(int(H), int(W)))]


def _gradient(image: torch.Tensor, eps: float, want_grad: bool, want_valid: bool):
    image = _check(image, "image")
    if image.dim() != 3:
        raise ValueError(f"image must be [C, H, W], got {tuple(image.shape)}")
    c, h, w = (int(s) for s in image.shape)
    if c < 1 or h < 2 or w < 2:
        raise ValueError(f"image must have a channel and at least 2 x 2 pixels (reflect padding), got {tuple(image.shape)}")
    dev = image.device
    gv = torch.empty_like(image) if want_grad else None
    gh = torch.empty_like(image) if want_grad else None
    valid = torch.empty(image.shape, dtype=torch.bool, device=dev) if want_valid else None
    with torch.cuda.device(dev):
        st = _native.load().splatraster_image_gradient(1, c, h, w, ptr(image), float(eps), ptr(gv), ptr(gh), ptr(valid), _stream(dev))
    _native.check(st, "splatraster_image_gradient")
    return gv, gh, valid


def image_gradient(image: torch.Tensor):
    """utils/utils.py image_gradient: (grad_v, grad_h) of every channel of image [C,H,W], Scharr kernels over 32, reflect padding"""
    gv, gh, _ = _gradient(image, 0.0, True, False)
    return gv, gh


def image_gradient_mask(image: torch.Tensor, eps: float = 0.01):
    """utils/utils.py image_gradient_mask: (mask_v, mask_h), bool [C,H,W]: all nine padded neighbours have |p| > eps.  The two are
    the same tensor's values (the reference computes the same mask twice)"""
    _, _, valid = _gradient(image, eps, False, True)
    return valid, valid.clone()


def compute_grad_masks(images: torch.Tensor, edge_threshold: float, dataset_type: str, return_intensity: bool = False,
                       return_thresholds: bool = False, eps: float = 0.01):
    """Camera.compute_grad_mask for a batch: images [N,3,H,W] -> masks [N,1,H,W], float32 for dataset_type "replica" (0 / 1 inside the
    32 x 32 blocks, the raw intensity in the remainder rows / columns and in blocks that hold a NaN), bool otherwise.  Optionally also the
    gradient intensity [N,1,H,W] and the thresholds ([N,32,32] per block for "replica", [N] otherwise).  One launch sequence, no host
    synchronisation."""
    images = _check(images, "images")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images must be [N, 3, H, W], got {tuple(images.shape)}")
    n, _, h, w = (int(s) for s in images.shape)
    if n < 1:
        raise ValueError("images holds no frame")
    replica = dataset_type == "replica"
    if replica and (h < BLOCKS or w < BLOCKS):
        raise ValueError(f"the replica branch needs frames of at least {BLOCKS} x {BLOCKS} pixels (the reference takes the median of an "
                         f"empty block and raises), got {h} x {w}")
    if h < 2 or w < 2:
        raise ValueError(f"frames must be at least 2 x 2 pixels (reflect padding), got {h} x {w}")
    dev = images.device
    lib = _native.load()
    mode = REPLICA if replica else GLOBAL
    out = torch.empty((n, 1, h, w), dtype=torch.float32 if replica else torch.bool, device=dev)
    intensity = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev) if return_intensity else None
    thresholds = torch.empty((n, BLOCKS, BLOCKS) if replica else (n,), dtype=torch.float32, device=dev) if return_thresholds else None
    nb = C.c_size_t(0)
    _native.check(lib.splatraster_grad_mask_workspace_bytes(n, h, w, mode, int(return_intensity), C.byref(nb)),
                  "splatraster_grad_mask_workspace_bytes")
    with torch.cuda.device(dev):
        ws = workspace(nb.value, dev)
        st = lib.splatraster_grad_mask(n, h, w, ptr(images), float(edge_threshold), float(eps), mode, 0 if replica else 1, ptr(out),
                                       ptr(intensity), ptr(thresholds), ptr(ws), ws.numel(), _stream(dev))
    _native.check(st, "splatraster_grad_mask")
    res = (out,) + ((intensity,) if return_intensity else ()) + ((thresholds,) if return_thresholds else ())
    return res if len(res) > 1 else out


def compute_grad_mask(viewpoint_or_image, config):
    """Drop-in body of Camera.compute_grad_mask(config): reads config["Training"]["edge_threshold"] and config["Dataset"]["type"].  Given a
    camera (anything with `original_image` [3,H,W]) it sets `grad_mask` on it, as the reference does, and returns the mask; given an image
    [3,H,W] it returns the mask [1,H,W]."""
    edge_threshold = config["Training"]["edge_threshold"]
    image = viewpoint_or_image if isinstance(viewpoint_or_image, torch.Tensor) else viewpoint_or_image.original_image
    if not isinstance(image, torch.Tensor) or image.dim() != 3:
        raise ValueError("compute_grad_mask needs an image [3, H, W] or a camera whose original_image is one")
    mask = compute_grad_masks(image[None], edge_threshold, config["Dataset"]["type"])[0]
    if not isinstance(viewpoint_or_image, torch.Tensor):
        viewpoint_or_image.grad_mask = mask
    return mask


def _select(values, rows: int, positive_only: bool, opacity, opacity_min: float, mask, want_std: bool, want_valid: bool):
    dev = values.device
    n = values.numel() // rows
    lib = _native.load()
    median = torch.empty(rows, dtype=torch.float32, device=dev)
    std = torch.empty(rows, dtype=torch.float32, device=dev) if want_std else None
    valid = torch.empty(values.shape, dtype=torch.bool, device=dev) if want_valid else None
    nb = C.c_size_t(0)
    _native.check(lib.splatraster_masked_median_workspace_bytes(rows, n, C.byref(nb)), "splatraster_masked_median_workspace_bytes")
    with torch.cuda.device(dev):
        ws = workspace(nb.value, dev)
        st = lib.splatraster_masked_median(rows, n, ptr(values), int(positive_only), ptr(opacity), float(opacity_min), ptr(mask),
                                           ptr(median), ptr(std), None, ptr(valid), ptr(ws), ws.numel(), _stream(dev))
    _native.check(st, "splatraster_masked_median")
    return median, std, valid


def _same_shape(t, like, name):
    if t.shape != like.shape:
        raise ValueError(f"{name} must have the shape of the values {tuple(like.shape)}, got {tuple(t.shape)}")


def get_median_depth(depth, opacity=None, mask=None, return_std=False):
    """utils/utils.py get_median_depth: the lower median of depth[(depth > 0) & (opacity > 0.95) & mask] (0-dim), with return_std also the
    unbiased standard deviation and the selection (bool, depth's shape).  An empty selection gives NaN for both (the reference raises;
    raising would need a read-back); `opacity` may be left out (the reference's signature allows it, its body does not)."""
    depth = _check(depth, "depth")
    if opacity is not None:
        opacity = _check(opacity, "opacity")
        _same_shape(opacity, depth, "opacity")
    if mask is not None:
        mask = _check(mask, "mask", torch.bool)
        _same_shape(mask, depth, "mask")
    median, std, valid = _select(depth, 1, True, opacity, 0.95, mask, bool(return_std), bool(return_std))
    if return_std:
        return median[0], std[0], valid
    return median[0]


def masked_median(values, valid=None):
    """Lower median of every row of values [N, ...] over the elements where `valid` (bool, same shape; None: all) holds: [N] float32,
    NaN for a row without a valid element or with a valid NaN.  Negative values order correctly."""
    values = _check(values, "values")
    if values.dim() < 1 or values.shape[0] < 1:
        raise ValueError(f"values must be [N, ...] with N >= 1, got {tuple(values.shape)}")
    if valid is not None:
        valid = _check(valid, "valid", torch.bool)
        _same_shape(valid, values, "valid")
    return _select(values, int(values.shape[0]), False, None, 0.0, valid, False, False)[0]
