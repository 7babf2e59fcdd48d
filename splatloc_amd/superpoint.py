"""The SuperPoint head on the device: everything behind the network's two convolution heads.

`semi` [B,65,Hc,Wc] (the logits of convPb) and `coarse` [B,256,Hc,Wc] (the output of convDb) go in; the score map, its
non-maximum suppression, the keypoints under the threshold / border / max_keypoints rules and their descriptors come out, and so
do the dense descriptor image that fusion.integrate_frames averages and the sp_kp_mask that map_step and
matching.frustum_candidates read.  hloc's SuperPoint is not part of the reference tree; include/splatraster.h (splatraster_sp_*)
and INTEGRATION.md §24 hold the definitions this module implements.

Everything is the HIP of csrc/superpoint_head.hip behind the C ABI, on the current stream and without a host synchronisation:
the number of candidates decides the order of the keypoints on the device.  Only `postprocess` reads the counts back (one read
for the batch) to cut the padded outputs to hloc's shapes.  Inputs are float32 contiguous device tensors; anything else raises
before device work.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native
from ._host import _stream, ptr, workspace

CELL = 8
DESC_DIM = 256
MAX_RADIUS = 8
MAX_KEYPOINTS = 65535


def _check(t, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}; the SuperPoint head runs on a ROCm device only (there is no CPU fallback)")
    if t.dtype is not dtype:
        raise ValueError(f"{name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach()


def _check_semi(semi) -> torch.Tensor:
    semi = _check(semi, "semi")
    if semi.dim() != 4 or semi.shape[1] != 65 or min(semi.shape) < 1:
        raise ValueError(f"semi must be [B, 65, Hc, Wc], got {tuple(semi.shape)}")
    return semi


def _check_coarse(coarse) -> torch.Tensor:
    coarse = _check(coarse, "coarse")
    if coarse.dim() != 4 or coarse.shape[1] != DESC_DIM or min(coarse.shape) < 1:
        raise ValueError(f"coarse must be [B, {DESC_DIM}, Hc, Wc], got {tuple(coarse.shape)}")
    return coarse


def _check_map(t, name: str) -> torch.Tensor:
    t = _check(t, name)
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name} must be [B, H, W], got {tuple(t.shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{name} has {t.numel()} pixels; the stage indexes fewer than 2^31")
    return t


def _check_radius(radius) -> int:
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"nms radius must be in 0..{MAX_RADIUS}, got {radius}")
    return radius


def _check_selection(keypoint_threshold, max_keypoints, remove_borders):
    threshold, k, border = float(keypoint_threshold), int(max_keypoints), int(remove_borders)
    if not threshold >= 0.0:
        raise ValueError(f"keypoint_threshold must be >= 0, got {keypoint_threshold}")
    if not 1 <= k <= MAX_KEYPOINTS:
        raise ValueError(f"max_keypoints must be in 1..{MAX_KEYPOINTS}, got {max_keypoints}")
    if border < 0:
        raise ValueError(f"remove_borders must be >= 0, got {remove_borders}")
    return threshold, k, border


def _workspace(b: int, h: int, w: int, k: int, dev) -> torch.Tensor:
    nb = C.c_size_t(0)
    _native.check(_native.load().splatraster_sp_workspace_bytes(b, h, w, k, C.byref(nb)), "splatraster_sp_workspace_bytes")
    return workspace(nb.value, dev)


def nms_tile():
    """(tile_h, tile_w): the outputs one NMS workgroup owns at radii 0..4; at radii 5..8 the tiles have half that side, so every
    edge of this tile is a tile edge at every radius.  Host only."""
    th, tw = C.c_int32(0), C.c_int32(0)
    _native.check(_native.load().splatraster_sp_nms_tile(C.byref(th), C.byref(tw)), "splatraster_sp_nms_tile")
    return int(th.value), int(tw.value)


def _scores(semi: torch.Tensor) -> torch.Tensor:
    b, _, hc, wc = (int(s) for s in semi.shape)
    out = torch.empty((b, CELL * hc, CELL * wc), dtype=torch.float32, device=semi.device)
    with torch.cuda.device(semi.device):
        st = _native.load().splatraster_sp_scores(b, hc, wc, ptr(semi), ptr(out), _stream(semi.device))
    _native.check(st, "splatraster_sp_scores")
    return out


def nms(scores: torch.Tensor, radius: int = 4) -> torch.Tensor:
    """N [B,H,W] of scores [B,H,W]: three rounds of max-pool suppression with a (2 radius + 1)^2 window clipped to the image; the
    survivors keep their score, everything else is 0.  radius 0 returns a copy."""
    scores = _check_map(scores, "scores")
    radius = _check_radius(radius)
    b, h, w = (int(s) for s in scores.shape)
    out = torch.empty_like(scores)
    with torch.cuda.device(scores.device):
        st = _native.load().splatraster_sp_nms(b, h, w, ptr(scores), radius, ptr(out), _stream(scores.device))
    _native.check(st, "splatraster_sp_nms")
    return out


def score_map(semi: torch.Tensor, nms_radius: int = 4) -> torch.Tensor:
    """N [B,8 Hc,8 Wc]: softmax over semi's 65 channels, dustbin dropped, depth-to-space, then `nms` (radius 0: the raw scores S)."""
    semi = _check_semi(semi)
    radius = _check_radius(nms_radius)
    s = _scores(semi)
    return s if radius == 0 else nms(s, radius)


def _select(n_map: torch.Tensor, threshold: float, k: int, border: int, ws: torch.Tensor):
    b, h, w = (int(s) for s in n_map.shape)
    dev = n_map.device
    keypoints = torch.empty((b, k, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((b, k), dtype=torch.float32, device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    candidates = torch.empty(b, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _native.load().splatraster_sp_select(b, h, w, ptr(n_map), threshold, k, border, ptr(keypoints), ptr(scores), ptr(count),
                                                  ptr(candidates), ptr(ws), ws.numel(), _stream(dev))
    _native.check(st, "splatraster_sp_select")
    return keypoints, scores, count, candidates


def select(nms_scores: torch.Tensor, keypoint_threshold: float = 0.005, max_keypoints: int = 4096, remove_borders: int = 4):
    """Keypoints of N [B,H,W]: the pixels with N > keypoint_threshold at least remove_borders pixels inside the image.  Returns
    (keypoints [B,K,2] as (x, y), scores [B,K], count [B] int32, candidates [B] int32) with K = max_keypoints, count = min(n, K)
    and rows at and beyond count zero.  An image with n <= K candidates lists them in row-major order; one with more lists its K
    largest scores in descending order, equal scores by ascending row-major index."""
    n_map = _check_map(nms_scores, "nms_scores")
    threshold, k, border = _check_selection(keypoint_threshold, max_keypoints, remove_borders)
    b, h, w = (int(s) for s in n_map.shape)
    return _select(n_map, threshold, k, border, _workspace(b, h, w, k, n_map.device))


def _sample(coarse: torch.Tensor, keypoints: torch.Tensor, count: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    b, _, hc, wc = (int(s) for s in coarse.shape)
    k = int(keypoints.shape[1])
    desc = torch.empty((b, DESC_DIM, k), dtype=torch.float32, device=coarse.device)
    with torch.cuda.device(coarse.device):
        st = _native.load().splatraster_sp_sample(b, hc, wc, ptr(coarse), k, ptr(keypoints), ptr(count), ptr(desc), ptr(ws), ws.numel(),
                                                  _stream(coarse.device))
    _native.check(st, "splatraster_sp_sample")
    return desc


def sample(coarse: torch.Tensor, keypoints: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """descriptors [B,256,K] of keypoints [B,K,2] (pixel (x, y), not necessarily integers): coarse normalised over its channels,
    interpolated bilinearly (align_corners, zero padding) and normalised again.  Columns at and beyond count[b] are zero."""
    coarse = _check_coarse(coarse)
    keypoints = _check(keypoints, "keypoints")
    count = _check(count, "count", torch.int32)
    b, _, hc, wc = (int(s) for s in coarse.shape)
    if keypoints.dim() != 3 or keypoints.shape[0] != b or keypoints.shape[2] != 2 or not 1 <= keypoints.shape[1] <= MAX_KEYPOINTS:
        raise ValueError(f"keypoints must be [{b}, K, 2] with K in 1..{MAX_KEYPOINTS}, got {tuple(keypoints.shape)}")
    if tuple(count.shape) != (b,):
        raise ValueError(f"count must be [{b}], got {tuple(count.shape)}")
    if not (coarse.device == keypoints.device == count.device):
        raise ValueError("coarse, keypoints and count must be on one device")
    return _sample(coarse, keypoints, count, _workspace(b, CELL * hc, CELL * wc, int(keypoints.shape[1]), coarse.device))


def detect(semi: torch.Tensor, coarse: torch.Tensor, nms_radius: int = 4, keypoint_threshold: float = 0.005, max_keypoints: int = 4096,
           remove_borders: int = 4) -> dict:
    """`score_map`, `select` and `sample` as one launch sequence on one workspace, bit-identical to the staged calls.  Returns the
    padded device tensors {"keypoints" [B,K,2], "scores" [B,K], "descriptors" [B,256,K], "count" [B], "candidates" [B],
    "dense_scores" [B,H,W] = N}; nothing is read back."""
    semi = _check_semi(semi)
    coarse = _check_coarse(coarse)
    radius = _check_radius(nms_radius)
    threshold, k, border = _check_selection(keypoint_threshold, max_keypoints, remove_borders)
    if coarse.device != semi.device or coarse.shape[0] != semi.shape[0] or coarse.shape[2:] != semi.shape[2:]:
        raise ValueError(f"semi {tuple(semi.shape)} on {semi.device} and coarse {tuple(coarse.shape)} on {coarse.device} do not belong "
                         "to one batch")
    b, _, hc, wc = (int(s) for s in semi.shape)
    ws = _workspace(b, CELL * hc, CELL * wc, k, semi.device)
    s = _scores(semi)
    n_map = s if radius == 0 else nms(s, radius)
    keypoints, scores, count, candidates = _select(n_map, threshold, k, border, ws)
    desc = _sample(coarse, keypoints, count, ws)
    return {"keypoints": keypoints, "scores": scores, "descriptors": desc, "count": count, "candidates": candidates,
            "dense_scores": n_map}


def postprocess(semi: torch.Tensor, coarse: torch.Tensor, nms_radius: int = 4, keypoint_threshold: float = 0.005,
                max_keypoints: int = 4096, remove_borders: int = 4, original_size=None) -> list:
    """`detect`, cut to hloc's per-image dicts: {"keypoints" [n,2], "scores" [n], "descriptors" [256,n], "dense_scores" [H,W]} for
    every image of the batch.  One host read (the counts of the whole batch).  original_size = (width, height) of the image before
    it was resized to the network's input, or one such pair per image: the keypoints are rescaled as test.py does,
    (kp + .5) * scale - .5 with scale = original / network size."""
    out = detect(semi, coarse, nms_radius, keypoint_threshold, max_keypoints, remove_borders)
    b, h, w = (int(s) for s in out["dense_scores"].shape)
    sizes = None
    if original_size is not None:
        sizes = torch.as_tensor(original_size, dtype=torch.float32).reshape(-1, 2)
        if sizes.shape[0] not in (1, b):
            raise ValueError(f"original_size must be (width, height) or one pair per image, got {tuple(sizes.shape)}")
        sizes = sizes.expand(b, 2)
    counts = out["count"].tolist()   # the one host read
    res = []
    for i, n in enumerate(counts):
        kp = out["keypoints"][i, :n]
        if sizes is not None:
            scale = (sizes[i] / torch.tensor([float(w), float(h)])).to(kp.device)
            kp = (kp + 0.5) * scale - 0.5
        res.append({"keypoints": kp, "scores": out["scores"][i, :n], "descriptors": out["descriptors"][i, :, :n],
                    "dense_scores": out["dense_scores"][i]})
    return res


def sp_kp_mask(dense_scores: torch.Tensor, threshold: float = 0.005) -> torch.Tensor:
    """dataset.py:163: the keypoint mask of a suppressed score map, dense_scores > threshold (bool, same shape)."""
    return _check(dense_scores, "dense_scores") > float(threshold)


def dense_descriptors(coarse: torch.Tensor, rows=None, out: torch.Tensor = None) -> torch.Tensor:
    """The descriptor of `sample` at every pixel: [B,rows,W,256] float32, channel-last, the layout fusion.integrate_frames reads.
    rows = (first, stop) bounds the image rows (and the memory: a 480 x 640 frame is 315 MB); None: all H = 8 Hc of them.  `out`
    may hold the result.  Bit-identical to `sample` at the same pixel."""
    coarse = _check_coarse(coarse)
    b, _, hc, wc = (int(s) for s in coarse.shape)
    h, w = CELL * hc, CELL * wc
    r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= h:
        raise ValueError(f"rows must be (first, stop) with 0 <= first < stop <= {h}, got {rows}")
    shape = (b, r1 - r0, w, DESC_DIM)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=coarse.device)
    else:
        _check(out, "out")
        if tuple(out.shape) != shape or out.device != coarse.device:
            raise ValueError(f"out must be {shape} on {coarse.device}, got {tuple(out.shape)} on {out.device}")
    ws = _workspace(b, h, w, 1, coarse.device)
    with torch.cuda.device(coarse.device):
        st = _native.load().splatraster_sp_dense_descriptors(b, hc, wc, ptr(coarse), r0, r1 - r0, ptr(out), ptr(ws), ws.numel(),
                                                             _stream(coarse.device))
    _native.check(st, "splatraster_sp_dense_descriptors")
    return out
