"""Host plumbing between torch tensors and the C ABI (include/splatraster.h): pointers, the current stream and device, input
preparation and workspaces.  Every module that calls the library through ctypes takes these from here; `rasterizer.py`
re-exports the underscore names it used to define.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr(t: Optional[torch.Tensor]):
    """`_ptr` that also maps a zero-element tensor to NULL (the stage entry points take NULL for an empty argument); the raster
    hot path keeps `_ptr` and its one attribute access"""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _prep(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """contiguous fp32 on `device`, 16-byte aligned (kernels use 128-bit loads).  The common case — the
    tensor already is all that — costs three attribute checks (host time is what bounds small frames)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype is torch.float32 and t.device == device and t.is_contiguous() and not (t.data_ptr() & 15):
        return t.detach() if t.requires_grad else t
    t = t.detach()
    if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


_EMPTY: dict = {}


def _empty(device) -> torch.Tensor:
    """one shared zero-element placeholder per device for the `None` slots of save_for_backward"""
    e = _EMPTY.get(device)
    if e is None:
        e = _EMPTY[device] = torch.empty(0, device=device)
    return e


class _on_device:
    """`with torch.cuda.device(dev)` only when `dev` is not already current (the context manager costs ~10 us)."""

    def __init__(self, device):
        self.ctx = None if torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> C.c_void_p:
    """the hipStream_t torch would launch on right now (device's current stream).  The raw getter costs ~0.3 us; building a
    torch.cuda.Stream object ~8 us — five of those per refinement iteration were 10 % of its host time."""
    if _RAW_STREAM is not None:
        idx = device.index
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device() if idx is None else idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"splatloc_amd rasterizer: `{name}` is on {t.device}; tensors must be on a ROCm device "
            "(the HIP kernels are the only implementation, there is no CPU fallback)")


def device(what: str) -> torch.device:
    """the current HIP device; without one, `what` (a stage's name for itself) goes into the error"""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} runs on the GPU: no HIP device is available")
    return torch.device("cuda", torch.cuda.current_device())


def float_tensor(a, what, dtypes=(torch.float32, torch.float64)):
    """numpy / torch array of one of `dtypes` -> torch tensor (no device move)"""
    names = [str(d).replace("torch.", "") for d in dtypes]
    allowed = ", ".join(names[:-1]) + " or " + names[-1]
    if isinstance(a, np.ndarray):
        if a.dtype not in tuple(getattr(np, n) for n in names):
            raise ValueError(f"{what} must be {allowed}, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a))
    t = torch.as_tensor(a)
    if t.dtype not in dtypes:
        raise ValueError(f"{what} must be {allowed}, got {t.dtype}")
    return t


def workspace(nbytes, dev) -> torch.Tensor:
    """uint8 scratch of a `*_workspace_bytes` query (never zero elements: the entry points refuse a NULL workspace)"""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
