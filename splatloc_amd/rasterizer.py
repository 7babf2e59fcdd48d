"""Host-side mirror of the `diff_gauss` extension API.

Names, argument meaning and error behaviour follow what SplatLoc calls at
gaussian_splatting/gaussian_renderer/__init__.py:42-57,117-126 (the extension's own
Python wrapper is un-vendored): `GaussianRasterizationSettings`
(12-field NamedTuple), `GaussianRasterizer(nn.Module)` whose forward returns the 4-tuple
`(color[C,H,W], depth[1,H,W], alpha[1,H,W], radii[P] int32)`, `rasterize_gaussians` and the
`_RasterizeGaussians` autograd.Function; `rasterize_window` / `_RasterizeWindow` for the views of a window as one launch
sequence.  The launches themselves are plain functions (`view_forward` / `view_backward`, `window_forward` /
`window_backward` / `window_backward_cameras`), which the autograd Functions adapt and the graph-free loops call directly.

All compute is in the HIP library behind include/splatraster.h; tensors must live on a
ROCm device.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _native
from ._host import _empty, _on_device, _prep, _ptr, _require_gpu, _stream  # noqa: F401 (re-exported)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _no_backward_follows(*inputs) -> bool:
    """Decided where the grad mode is still visible, in front of Function.apply: inside Function.forward grad mode is off and
    `ctx.needs_input_grad` only repeats every input's own `requires_grad` — true for trained parameters rendered under
    torch.no_grad() (evaluation renders), where no graph is recorded and no backward can follow."""
    return not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs))


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    # the camera tensors are passed as explicit autograd inputs as well, so that a pose
    # parametrisation upstream of viewmatrix / projmatrix / campos receives gradients
    # (pose-gradient extension; the reference has no such path)
    rs = raster_settings
    tensors = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.campos)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, rs.viewmatrix, rs.projmatrix, rs.campos,
                                     _no_backward_follows(*tensors))


# A forward returns a FRAME (SimpleNamespace): its outputs and everything its backward reads, by name.  An autograd adapter
# saves the frame's prepared inputs, its buffers in `_BUFFERS` order and more inputs after them, and rebuilds the frame from
# them in its backward.  The saved order is the one earlier revisions had (code that indexes saved_tensors keeps working):
# per view `_VIEW_INPUTS`, buffers; per window `_WINDOW_INPUTS`, buffers, (view, proj, campos) of every view, bg.
_BUFFERS = ("radii", "geom", "binning", "img", "color", "depth", "alpha")
_VIEW_INPUTS = ("m3", "shs", "col", "opa", "sca", "rot", "cov", "bg", "view", "proj", "campos")
_WINDOW_INPUTS = ("m3", "col", "opa", "sca", "rot", "cov")


def _save(ctx, frame, inputs, after=(), buffers=_BUFFERS) -> None:
    none = _empty(frame.dev)
    ctx.n_saved_inputs = len(inputs)
    ctx.save_for_backward(*[none if t is None else t for t in inputs], *[getattr(frame, k) for k in buffers],
                          *[none if t is None else t for t in after])


def _saved(node, buffers=_BUFFERS):
    """(inputs then `after` — None for a placeholder: a prepared input is never empty —, {buffer name: tensor}) saved by
    `_save`"""
    s, n, m = node.saved_tensors, node.n_saved_inputs, len(buffers)
    return [t if t.numel() else None for t in s[:n] + s[n + m:]], dict(zip(buffers, s[n:n + m]))


_PIECES = ("m3", "op", "col", "sca", "rot", "cov", "sh")


def _grad_layout(P: int, Cn: int, col=True, sca=True, rot=True, cov=False, sh=None):
    """The ONE allocation of a forward's parameter gradients: 16-byte aligned pieces in `_PIECES` order, the absent ones
    left out.  Returns (shapes, offsets, total_floats)."""
    shapes = {"m3": (P, 3), "op": (P, 1)}
    for k, on, shp in (("col", col, (P, Cn)), ("sca", sca, (P, 3)), ("rot", rot, (P, 4)), ("cov", cov, (P, 6)),
                       ("sh", sh is not None, sh)):
        if on:
            shapes[k] = tuple(shp)
    offs, total = {}, 0
    for k, shp in shapes.items():
        offs[k] = total
        total += (math.prod(shp) + 3) & ~3
    return shapes, offs, total


def _grad_pieces(flat: torch.Tensor, shapes: dict, offs: dict) -> dict:
    return {k: flat[offs[k]:offs[k] + math.prod(shapes[k])].view(shapes[k]) if k in shapes else None for k in _PIECES}


def view_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                 raster_settings: GaussianRasterizationSettings, viewmatrix=None, projmatrix=None, campos=None, forward_only=False):
    """One view: splatraster_forward_geometry + splatraster_forward_render.  The camera tensors default to the settings'.
    `forward_only`: no backward will read the frame (Settings.debug bit SETTINGS_FORWARD_ONLY: the wide forward writes no dead marks).
    Returns the frame: dev, P, st, num_rendered, the prepared inputs (`_VIEW_INPUTS`, None when absent) and the buffers
    radii [P], geom, binning, img, color [C,H,W], depth [1,H,W], alpha [1,H,W]."""
    lib = _native.load()
    _require_gpu(means3D, "means3D")
    dev = means3D.device
    rs = raster_settings
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)

    m3 = _prep(means3D, dev)
    shs = _prep(sh, dev)
    col = _prep(colors_precomp, dev)
    opa = _prep(opacities, dev)
    sca = _prep(scales, dev)
    rot = _prep(rotations, dev)
    cov = _prep(cov3Ds_precomp, dev)
    bg = _prep(rs.bg, dev)
    view = _prep(rs.viewmatrix if viewmatrix is None else viewmatrix, dev)
    proj = _prep(rs.projmatrix if projmatrix is None else projmatrix, dev)
    campos = _prep(rs.campos if campos is None else campos, dev)

    if shs is not None:
        Cn, M = 3, int(shs.shape[1])
    elif col is not None:
        Cn, M = int(col.shape[1]), 0
    elif colors_precomp is not None and colors_precomp.dim() == 2 and colors_precomp.shape[1] > 0:
        Cn, M = int(colors_precomp.shape[1]), 0     # P = 0: the channel count is still the table's width
    else:
        Cn, M = (3, 0)
    st = _native.Settings(H, W, float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier),
                          int(rs.sh_degree), M, Cn, 0 if bg is None else int(bg.numel()),
                          int(bool(rs.prefiltered)), int(bool(rs.debug)) | (_native.SETTINGS_FORWARD_ONLY if forward_only else 0))

    color = torch.empty((Cn, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)   # preprocess_kernel writes every element
    geom = torch.empty((lib.splatraster_geometry_bytes(P),), dtype=torch.uint8, device=dev)
    img = torch.empty((lib.splatraster_image_bytes(W, H),), dtype=torch.uint8, device=dev)
    stream = _stream(dev)
    R = C.c_int64(0)
    with _on_device(dev):
        _native.check(lib.splatraster_forward_geometry(
            C.byref(st), P, _ptr(m3), _ptr(shs), _ptr(opa), _ptr(sca), _ptr(rot), _ptr(cov), _ptr(view),
            _ptr(proj), _ptr(campos), _ptr(geom), _ptr(radii), C.byref(R), stream), "forward_geometry")
        binning = torch.empty((lib.splatraster_binning_bytes(P, R.value, W, H, Cn),), dtype=torch.uint8,
                              device=dev)
        _native.check(lib.splatraster_forward_render(
            C.byref(st), P, R.value, _ptr(bg), _ptr(col), _ptr(geom), _ptr(binning), _ptr(img),
            _ptr(color), _ptr(depth), _ptr(alpha), stream), "forward_render")
    return SimpleNamespace(dev=dev, P=P, st=st, num_rendered=int(R.value), m3=m3, shs=shs, col=col, opa=opa, sca=sca, rot=rot,
                           cov=cov, bg=bg, view=view, proj=proj, campos=campos, radii=radii, geom=geom, binning=binning, img=img,
                           color=color, depth=depth, alpha=alpha)


def view_backward(f, grad_color, grad_depth=None, grad_alpha=None, want_pose: bool = False) -> dict:
    """splatraster_backward of the frame `f` of `view_forward`; an output gradient that is None did not reach the loss.
    Returns the gradients by name: m3, op, col, sca, rot, cov, sh (None for an absent input), m2 (dL/dmeans2D) and, with
    `want_pose`, view, proj, campos (else None)."""
    lib = _native.load()
    dev, P, st = f.dev, f.P, f.st
    g_color = _prep(grad_color, dev)
    if g_color is None:
        g_color = torch.zeros_like(f.color)
    g_depth, g_alpha = _prep(grad_depth, dev), _prep(grad_alpha, dev)

    f32 = dict(dtype=torch.float32, device=dev)
    # every parameter gradient of the frame is carved out of ONE allocation, so a frame-parallel replica can all-reduce
    # them where they are as a single RCCL call (frame_parallel.allreduce_grads); the viewspace gradient is per-view
    # state and stays outside
    shapes, offs, total = _grad_layout(P, st.channels, col=f.col is not None, sca=f.sca is not None, rot=f.rot is not None,
                                       cov=f.cov is not None, sh=None if f.shs is None else f.shs.shape)
    d = _grad_pieces(torch.empty((total,), **f32), shapes, offs)
    d["m2"] = torch.empty((P, 3), **f32)
    d["view"] = torch.empty((4, 4), **f32) if want_pose else None
    d["proj"] = torch.empty((4, 4), **f32) if want_pose else None
    d["campos"] = torch.empty((3,), **f32) if (want_pose and f.campos is not None) else None   # (written in full by the backward)
    with _on_device(dev):
        _native.check(lib.splatraster_backward(
            C.byref(st), P, f.num_rendered, _ptr(f.bg), _ptr(f.m3), _ptr(f.shs), _ptr(f.col), _ptr(f.opa),
            _ptr(f.sca), _ptr(f.rot), _ptr(f.cov), _ptr(f.view), _ptr(f.proj), _ptr(f.campos), _ptr(f.radii),
            _ptr(f.geom), _ptr(f.binning), _ptr(f.img), _ptr(f.color), _ptr(f.depth), _ptr(f.alpha), _ptr(g_color),
            _ptr(g_depth), _ptr(g_alpha), _ptr(d["m3"]), _ptr(d["m2"]), _ptr(d["col"]), _ptr(d["op"]), _ptr(d["sca"]),
            _ptr(d["rot"]), _ptr(d["cov"]), _ptr(d["sh"]), _ptr(d["view"]), _ptr(d["proj"]), _ptr(d["campos"]), _stream(dev)),
            "backward")
    return d


class _RasterizeGaussians(torch.autograd.Function):
    """The autograd adapter of `view_forward` / `view_backward`; `grad_fn.num_rendered` is the frame's instance count."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings: GaussianRasterizationSettings, viewmatrix=None, projmatrix=None, campos=None, forward_only=False):
        # forward_only: no backward follows (_no_backward_follows, decided by the caller of apply); the render is told so
        f = view_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                         viewmatrix, projmatrix, campos, forward_only=bool(forward_only))
        ctx.dev, ctx.P, ctx.st, ctx.num_rendered = f.dev, f.P, f.st, f.num_rendered
        _save(ctx, f, [getattr(f, k) for k in _VIEW_INPUTS])
        ctx.mark_non_differentiable(f.radii)
        ctx.set_materialize_grads(False)   # no zero tensors for unused output gradients (radii, depth, alpha)
        return f.color, f.depth, f.alpha, f.radii

    @staticmethod
    def backward(ctx, grad_color, grad_depth, grad_alpha, _grad_radii=None):
        inputs, buffers = _saved(ctx)
        f = SimpleNamespace(dev=ctx.dev, P=ctx.P, st=ctx.st, num_rendered=ctx.num_rendered, **dict(zip(_VIEW_INPUTS, inputs)),
                            **buffers)
        want_pose = any(ctx.needs_input_grad[9:12]) if len(ctx.needs_input_grad) >= 12 else False
        d = view_backward(f, grad_color, grad_depth, grad_alpha, want_pose)
        # (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings,
        #  viewmatrix, projmatrix, campos, forward_only)
        return d["m3"], d["m2"], d["sh"], d["col"], d["op"], d["sca"], d["rot"], d["cov"], None, d["view"], d["proj"], d["campos"], None


def window_grad_layout(P: int, Cn: int, have_scales: bool = True, have_cov: bool = False):
    """Layout of the ONE allocation that holds the summed parameter gradients of a window: 16-byte aligned pieces
    `m3 [P,3] | op [P,1] | col [P,Cn] | sca [P,3] | rot [P,4] | cov [P,6]`, optionally followed by a `[2, P]` TAIL for the
    increments of xyz_gradient_accum / denom, so that a frame-parallel replica reduces gradients AND statistics as one
    in-place SUM (frame_parallel.reduce_step).  Returns (shapes, offsets, total_floats)."""
    return _grad_layout(P, Cn, sca=have_scales, rot=have_scales, cov=have_cov)


def window_grad_span(P: int, Cn: int, device, have_scales: bool = True, have_cov: bool = False, tail: bool = True,
                     zero: bool = False) -> dict:
    """Allocates the gradient allocation of `window_grad_layout` (+ the statistics tail).  `zero=True`: what a rank
    WITHOUT views in a frame-parallel step contributes — zero gradients in exactly the layout the other ranks' backward
    produced, so that every rank reduces the same buffer.  Keys: flat, tail ([2, P, 1] or None), m3, op, col, sca, rot, cov
    (and sh: None)."""
    shapes, offs, total = window_grad_layout(P, Cn, have_scales, have_cov)
    n = total + (2 * P if tail else 0)
    flat = (torch.zeros if zero else torch.empty)((n,), dtype=torch.float32, device=device)
    out = {"flat": flat, "tail": None, **_grad_pieces(flat, shapes, offs)}
    if tail:
        out["tail"] = flat[total:total + 2 * P].view(2, P, 1)
        if not zero:
            out["tail"].zero_()
    return out


def _window_compatible(settings) -> bool:
    """One launch sequence needs one image size, channel layout, scale modifier and background for all views."""
    if not settings:
        return True
    a = settings[0]
    for b in settings[1:]:
        if (int(b.image_height), int(b.image_width)) != (int(a.image_height), int(a.image_width)):
            return False
        if float(b.scale_modifier) != float(a.scale_modifier):
            return False
        if b.bg is not a.bg and b.bg.data_ptr() != a.bg.data_ptr() and not torch.equal(b.bg, a.bg):   # (the last test reads the device: only for distinct tensors)
            return False
    return True


def _split_head(split_last, Cn: int) -> int:
    """`split_last` (see _RasterizeWindow) as the number of leading colour channels of the first output; 0: no split."""
    head = Cn - 1 if split_last is True else (int(split_last) if (not isinstance(split_last, bool) and split_last) else 0)
    return head if Cn >= 2 and 1 <= head <= Cn - 1 else 0


def _window_views(f):
    """The WindowView array of a window frame: camera, tan-fov, radii and output planes of every view."""
    views = (_native.WindowView * f.V)()
    for v, (view, proj, campos) in enumerate(f.cams):
        w = views[v]
        w.viewmatrix, w.projmatrix = view.data_ptr(), proj.data_ptr()
        w.campos = None if campos is None else campos.data_ptr()
        w.tanfovx, w.tanfovy = f.tanfov[v]
        w.radii = f.radii[v].data_ptr() if f.P else None
        w.out_color, w.out_depth, w.out_alpha = f.color[v].data_ptr(), f.depth[v].data_ptr(), f.alpha[v].data_ptr()
    return views


class BoundedStatus:
    """A status block of the bounded window forward (splatraster_bounded_status_create) on `device`: R of the last sequence, the
    sticky overflow flag and the record of the first sequence that did not fit.  `read()` copies the host-mapped mirror (last_tag,
    then overflow, then the rest) and never synchronises; `clear()` is stream-ordered.  The owner calls `close()` once every
    stream that used the block has been synchronised (or uses it as a context manager, which synchronises the device first)."""

    def __init__(self, device):
        self.lib = _native.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BoundedStatus needs a GPU device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p()
        with _on_device(self.device):
            _native.check(self.lib.splatraster_bounded_status_create(C.byref(h)), "bounded_status_create")
        self.handle = h

    def read(self) -> _native.BoundedStatus:
        out = _native.BoundedStatus()
        _native.check(self.lib.splatraster_bounded_status_read(self.handle, C.byref(out)), "bounded_status_read")
        return out

    def clear(self) -> None:
        with _on_device(self.device):
            _native.check(self.lib.splatraster_bounded_status_clear(self.handle, _stream(self.device)), "bounded_status_clear")

    def close(self) -> None:
        if self.handle:
            self.lib.splatraster_bounded_status_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize(self.device)
        self.close()


class BoundedWindow:
    """What `window_forward(bounded=...)` renders into: a status block, the capacity (instances) the reusable `binning` tensor
    is laid out for, and the tag of the next sequence.  `reserve(capacity, ...)` (re)allocates `binning` for a frame shape —
    the only allocation of the mode, made when the shape or the capacity changes, never per frame.  A frame of more than
    `capacity` instances renders the background and sets the status block's sticky `overflow` (include/splatraster.h).
    `close()` frees a status block the window created itself (after the caller has synchronised the device)."""

    def __init__(self, device, capacity: int = 0, status: Optional[BoundedStatus] = None):
        self._own_status = status is None
        self.status = status if status is not None else BoundedStatus(device)
        self.device = self.status.device
        self.capacity = int(capacity)
        self.binning = None
        self.next_tag = 0
        self._shape = None

    def reserve(self, capacity: int, P: int, V: int, W: int, H: int, Cn: int) -> torch.Tensor:
        shape = (int(capacity), P, V, W, H, Cn)
        if self.binning is None or self._shape != shape:
            n = _native.load().splatraster_window_binning_bytes(P, V, int(capacity), W, H, Cn)
            self.binning = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self.capacity, self._shape = int(capacity), shape
        return self.binning

    def close(self) -> None:
        if self._own_status:
            self.status.close()


def window_forward(means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, raw=None, bounded=None,
                   forward_only=False):
    """The views of `settings` (1 <= V <= MAX_WINDOW_VIEWS, `_window_compatible`) as ONE launch sequence:
    splatraster_forward_window_geometry (+ _render).  Returns the frame: dev, P, V, st, R (instances per view), tanfov,
    the prepared inputs (`_WINDOW_INPUTS` and bg, None when absent), cams [(view, proj, campos)] per view and the buffers
    radii [V,P], geom, binning, img, color [V,C,H,W], depth [V,1,H,W], alpha [V,1,H,W].
    `raw` = (scaling [P,3], rotation [P,4], opacity [P,1], f_dc [P,1,3], extra [P,E] or None): RAW-parameter mode, in place of
    colors_precomp / opacities / scales / rotations (None): splatraster_forward_window_geometry_raw activates them inside the
    projection kernel and fills the frame's col [P,3+E], opa, sca, rot.
    `bounded` (a BoundedWindow): ONE call, splatraster_forward_window_bounded[_raw], into `bounded.binning` (laid out for
    `bounded.capacity` instances; reserved here on first use or when the shape changed) with the tag `bounded.next_tag`, which
    is then advanced: no host wait for the instance count and no allocation of `binning` per frame.  The frame's `R` is None
    (the count stays on the device: `bounded.status`), `capacity` is set, and `binning` is the shared tensor — valid until the
    next bounded forward.  Only where the binned front end runs: else RuntimeError ("unsupported configuration").
    `forward_only`: no backward will read the frame (Settings.debug bit SETTINGS_FORWARD_ONLY: the wide forward writes no dead marks)."""
    lib = _native.load()
    _require_gpu(means3D, "means3D")
    dev = means3D.device
    V = len(settings)
    assert 1 <= V <= _native.MAX_WINDOW_VIEWS
    rs0 = settings[0]
    P = int(means3D.shape[0])
    H, W = int(rs0.image_height), int(rs0.image_width)
    f32 = dict(dtype=torch.float32, device=dev)
    if raw is not None:     # the tensors the projection kernel fills
        E = 0 if raw[4] is None else int(raw[4].shape[1])
        scales, rotations, opacities = torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 1), **f32)
        colors_precomp = torch.empty((P, 3 + E), **f32)
    m3, col, opa = _prep(means3D, dev), _prep(colors_precomp, dev), _prep(opacities, dev)
    sca, rot, cov = _prep(scales, dev), _prep(rotations, dev), _prep(cov3Ds_precomp, dev)
    bg = _prep(rs0.bg, dev)
    Cn = int(colors_precomp.shape[1])
    st = _native.Settings(H, W, float(rs0.tanfovx), float(rs0.tanfovy), float(rs0.scale_modifier), 0, 0, Cn,
                          0 if bg is None else int(bg.numel()), 0, _native.SETTINGS_FORWARD_ONLY if forward_only else 0)
    # one allocation per kind; the per-view outputs are its slices (plain tensors for autograd: they do not
    # alias any input)
    f = SimpleNamespace(dev=dev, P=P, V=V, st=st, tanfov=[(float(rs.tanfovx), float(rs.tanfovy)) for rs in settings],
                        m3=m3, col=col, opa=opa, sca=sca, rot=rot, cov=cov, bg=bg,
                        cams=[(_prep(rs.viewmatrix, dev), _prep(rs.projmatrix, dev), _prep(rs.campos, dev)) for rs in settings],
                        color=torch.empty((V, Cn, H, W), **f32), depth=torch.empty((V, 1, H, W), **f32),
                        alpha=torch.empty((V, 1, H, W), **f32), radii=torch.empty((V, P), dtype=torch.int32, device=dev))
    views = _window_views(f)
    f.geom = torch.empty((lib.splatraster_window_geometry_bytes(P, V),), dtype=torch.uint8, device=dev)
    f.img = torch.empty((lib.splatraster_window_image_bytes(W, H, V),), dtype=torch.uint8, device=dev)
    stream = _stream(dev)
    R = (C.c_int64 * V)()
    f.capacity = None
    with _on_device(dev):
        if raw is not None:
            sc_r, ro_r, op_r, fd_r, ex_r = raw
            rf = _native.RawForward()
            rf.scaling, rf.rotation, rf.opacity, rf.f_dc = sc_r.data_ptr(), ro_r.data_ptr(), op_r.data_ptr(), fd_r.data_ptr()
            rf.extra = None if ex_r is None else ex_r.data_ptr()
            rf.extra_channels = E
            rf.scales, rf.rotations, rf.opacities, rf.colors = sca.data_ptr(), rot.data_ptr(), opa.data_ptr(), col.data_ptr()
        if bounded is not None:
            if bounded.device != (dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())):
                raise ValueError(f"window_forward: the bounded window lives on {bounded.device}, the tensors on {dev}")
            f.binning = bounded.reserve(bounded.capacity, P, V, W, H, Cn)
            f.R, f.capacity = None, bounded.capacity
            tag = bounded.next_tag & 0xFFFFFFFF
            bounded.next_tag += 1
            if raw is not None:
                _native.check(lib.splatraster_forward_window_bounded_raw(
                    C.byref(st), V, views, P, _ptr(m3), C.byref(rf), _ptr(bg), _ptr(f.geom), _ptr(f.binning), _ptr(f.img),
                    f.capacity, tag, bounded.status.handle, stream), "forward_window_bounded_raw")
            else:
                _native.check(lib.splatraster_forward_window_bounded(
                    C.byref(st), V, views, P, _ptr(m3), _ptr(opa), _ptr(sca), _ptr(rot), _ptr(cov), _ptr(bg), _ptr(col),
                    _ptr(f.geom), _ptr(f.binning), _ptr(f.img), f.capacity, tag, bounded.status.handle, stream),
                    "forward_window_bounded")
            return f
        if raw is not None:
            _native.check(lib.splatraster_forward_window_geometry_raw(
                C.byref(st), V, views, P, _ptr(m3), C.byref(rf), _ptr(f.geom), R, stream), "forward_window_geometry_raw")
        else:
            _native.check(lib.splatraster_forward_window_geometry(
                C.byref(st), V, views, P, _ptr(m3), _ptr(opa), _ptr(sca), _ptr(rot), _ptr(cov), _ptr(f.geom), R, stream),
                "forward_window_geometry")
        f.R = [int(r) for r in R]
        f.binning = torch.empty((lib.splatraster_window_binning_bytes(P, V, sum(f.R), W, H, Cn),), dtype=torch.uint8,
                                device=dev)
        _native.check(lib.splatraster_forward_window_render(
            C.byref(st), V, views, P, R, _ptr(bg), _ptr(col), _ptr(f.geom), _ptr(f.binning), _ptr(f.img), stream),
            "forward_window_render")
    return f


def _layout_counts(f):
    """num_rendered of a window frame's backward: the counts `binning` was laid out for — the per-view R, or for a bounded
    frame (R is None) {capacity, 0, ...}."""
    if f.R is None:
        return (C.c_int64 * f.V)(int(f.capacity), *([0] * (f.V - 1)))
    return (C.c_int64 * f.V)(*f.R)


def window_outputs(f, head: int = 0) -> list:
    """The per-view outputs of a window frame: (color, depth, alpha, radii), or with head > 0
    (color[:head], color[-1], depth, alpha, radii)."""
    Cn = f.st.channels
    if head:
        return [(f.color[v, :head], f.color[v, Cn - 1], f.depth[v], f.alpha[v], f.radii[v]) for v in range(f.V)]
    return [(f.color[v], f.depth[v], f.alpha[v], f.radii[v]) for v in range(f.V)]


def _window_grad_views(f, grads, head: int = 0, m2: Optional[torch.Tensor] = None):
    """`_window_views(f)` with the gradient planes of a backward filled in.  `grads`: per view (g_color, g_last, g_depth,
    g_alpha), None for an output that did not reach the loss — the colour plane is then ONE shared plane of zeros; `m2`
    [V,P,3]: where dL/dmeans2D goes.  Returns the array and the tensors that must outlive the call."""
    dev, st = f.dev, f.st
    views = _window_views(f)
    keep = []
    zeros_color = None
    for v, (g_color, g_last, g_depth, g_alpha) in enumerate(grads):
        g_color, g_last, g_depth, g_alpha = (_prep(g, dev) for g in (g_color, g_last, g_depth, g_alpha))
        if g_color is None:     # this view's colour buffer did not reach the loss
            if zeros_color is None:
                zeros_color = torch.zeros((st.channels, st.image_height, st.image_width), dtype=torch.float32, device=dev)
            g_color = zeros_color
        keep += [g_color, g_depth, g_alpha, g_last]
        w = views[v]
        w.dL_dout_color = g_color.data_ptr()
        w.dL_dout_depth = None if g_depth is None else g_depth.data_ptr()
        w.dL_dout_alpha = None if g_alpha is None else g_alpha.data_ptr()
        w.dL_dmeans2D = m2[v].data_ptr() if m2 is not None and f.P else None
        w.dL_dout_last = None if g_last is None else g_last.data_ptr()
        w.color_grad_channels = head
    return views, keep


def _camera_workspace(lib, V: int, dev, workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """The sets and tickets of the camera reduction of V views: the caller's tensor, checked, or a new one."""
    nws = lib.splatraster_window_camera_workspace_bytes(V)
    if workspace is None:
        workspace = torch.empty((nws,), dtype=torch.uint8, device=dev)
    assert workspace.numel() >= nws
    return workspace


def window_backward(f, grads, head: int = 0, grad_span: Optional[list] = None, raw=None, reg=None, cameras: bool = False,
                    workspace: Optional[torch.Tensor] = None) -> dict:
    """ONE backward for the views of `window_forward`'s frame `f`.  `grads`: per view (g_color, g_last, g_depth, g_alpha) of
    `window_outputs(f, head)`; None: that output did not reach the loss.  Returns the gradients summed over the views, by
    name: m3, op, col, sca, rot, cov (`window_grad_span` pieces) and m2 [V,P,3] (dL/dmeans2D per view).  `grad_span`: a
    list the allocation is appended to.  `raw` (window_forward's): splatraster_backward_window_raw chains through the
    activations inside the per-Gaussian kernel and returns scaling, rotation, opacity, f_dc, extra instead of col / op /
    sca / rot; `reg` = (row_grad [P], out [2], weight) joins the isotropic regulariser's term to dL/dscales there.
    `cameras`: splatraster_backward_window_joint — the same compositing backward, then ONE per-Gaussian kernel that also
    reduces the camera gradients of every view; the dict gains view [V,4,4], proj [V,4,4] and campos [V,3] (zeros: a window
    has precomputed colours only).  `workspace` as in `window_backward_cameras`.  Not with `raw` (ValueError)."""
    if cameras and raw is not None:
        raise ValueError("window_backward: cameras=True has no raw-parameter variant (pass the activated tensors to window_forward)")
    lib = _native.load()
    dev, V, P, st = f.dev, f.V, f.P, f.st
    Cn = st.channels
    f32 = dict(dtype=torch.float32, device=dev)
    # the summed parameter gradients of the window: 16-byte aligned pieces of ONE allocation, like the per-view
    # call, so a frame-parallel replica all-reduces them in place as a single RCCL call; with `grad_span` the
    # allocation ends with a zeroed [2, P] tail for the statistics increments, which then ride in the same call
    d = window_grad_span(P, Cn, dev, have_scales=f.sca is not None, have_cov=f.cov is not None, tail=grad_span is not None)
    if grad_span is not None:
        # only the whole allocation and its tail: holding the PIECES there would raise their use count and autograd's
        # AccumulateGrad would then deep-copy them instead of keeping them as the parameters' .grad
        grad_span.append({"flat": d["flat"], "tail": d["tail"]})
    d["m2"] = torch.empty((V, P, 3), **f32)
    views, keep = _window_grad_views(f, grads, head, d["m2"])
    R = _layout_counts(f)
    if cameras:
        d["view"], d["proj"], d["campos"] = (torch.empty(shp, **f32) for shp in ((V, 4, 4), (V, 4, 4), (V, 3)))
        workspace = _camera_workspace(lib, V, dev, workspace)
        with _on_device(dev):
            _native.check(lib.splatraster_backward_window_joint(
                C.byref(st), V, views, P, R, _ptr(f.bg), _ptr(f.m3), _ptr(f.col), _ptr(f.sca), _ptr(f.rot), _ptr(f.cov),
                _ptr(f.geom), _ptr(f.binning), _ptr(f.img), _ptr(d["m3"]), _ptr(d["col"]), _ptr(d["op"]), _ptr(d["sca"]),
                _ptr(d["rot"]), _ptr(d["cov"]), _ptr(workspace), _ptr(d["view"]), _ptr(d["proj"]), _ptr(d["campos"]),
                _stream(dev)), "backward_window_joint")
        return d
    if raw is None:
        with _on_device(dev):
            _native.check(lib.splatraster_backward_window(
                C.byref(st), V, views, P, R, _ptr(f.bg), _ptr(f.m3), _ptr(f.col), _ptr(f.sca), _ptr(f.rot), _ptr(f.cov),
                _ptr(f.geom), _ptr(f.binning), _ptr(f.img), _ptr(d["m3"]), _ptr(d["col"]), _ptr(d["op"]), _ptr(d["sca"]),
                _ptr(d["rot"]), _ptr(d["cov"]), _stream(dev)), "backward_window")
        return d
    sc_r, ro_r, op_r, fd_r, ex_r = raw
    E = 0 if ex_r is None else int(ex_r.shape[1])
    d["scaling"], d["rotation"], d["opacity"] = torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 1), **f32)
    d["f_dc"] = torch.empty(tuple(fd_r.shape), **f32)
    d["extra"] = torch.empty((P, E), **f32) if E else None
    rp = _native.RawParams()
    rp.scaling, rp.rotation, rp.opacity, rp.f_dc = sc_r.data_ptr(), ro_r.data_ptr(), op_r.data_ptr(), fd_r.data_ptr()
    rp.extra_channels = E
    rp.dL_dscaling, rp.dL_drotation = d["scaling"].data_ptr(), d["rotation"].data_ptr()
    rp.dL_dopacity, rp.dL_df_dc = d["opacity"].data_ptr(), d["f_dc"].data_ptr()
    rp.dL_dextra = None if d["extra"] is None else d["extra"].data_ptr()
    if reg is not None:
        rp.reg_row_grad, rp.reg_out, rp.reg_weight = reg[0].data_ptr(), reg[1].data_ptr(), float(reg[2])
    with _on_device(dev):
        _native.check(lib.splatraster_backward_window_raw(
            C.byref(st), V, views, P, R, _ptr(f.bg), _ptr(f.m3), _ptr(f.col), _ptr(f.sca), _ptr(f.rot), _ptr(f.geom),
            _ptr(f.binning), _ptr(f.img), C.byref(rp), _ptr(d["m3"]), _stream(dev)), "backward_window_raw")
    return d


def window_backward_cameras(f, grads, workspace: Optional[torch.Tensor] = None, out: Optional[dict] = None) -> dict:
    """The camera gradients of every view of `window_forward`'s frame `f`, and no parameter gradient
    (splatraster_backward_window_cameras: the compositing backward of `window_backward`, then one kernel over the (view,
    Gaussian) rows that writes nothing per Gaussian).  `grads`: per view (g_color [C,H,W], g_depth [1,H,W], g_alpha [1,H,W]);
    None: that output did not reach the loss.  Returns {"view": [V,4,4], "proj": [V,4,4], "campos": [V,3]} (campos: zeros, a
    window has precomputed colours only).  A loop passes `workspace` (uint8, splatraster_window_camera_workspace_bytes(V);
    zeroed by the call) and `out` (the dict of an earlier call, overwritten) to reuse them."""
    lib = _native.load()
    dev, V, P, st = f.dev, f.V, f.P, f.st
    if len(grads) != V:
        raise ValueError(f"window_backward_cameras: {len(grads)} gradient tuples for {V} views")
    f32 = dict(dtype=torch.float32, device=dev)
    d = out if out is not None else {"view": torch.empty((V, 4, 4), **f32), "proj": torch.empty((V, 4, 4), **f32),
                                     "campos": torch.empty((V, 3), **f32)}
    workspace = _camera_workspace(lib, V, dev, workspace)
    assert all(tuple(d[k].shape) == shp for k, shp in (("view", (V, 4, 4)), ("proj", (V, 4, 4)), ("campos", (V, 3))))
    views, keep = _window_grad_views(f, [(g_color, None, g_depth, g_alpha) for g_color, g_depth, g_alpha in grads])
    R = _layout_counts(f)
    with _on_device(dev):
        _native.check(lib.splatraster_backward_window_cameras(
            C.byref(st), V, views, P, R, _ptr(f.bg), _ptr(f.m3), _ptr(f.col), _ptr(f.sca), _ptr(f.rot), _ptr(f.cov),
            _ptr(f.geom), _ptr(f.binning), _ptr(f.img), _ptr(workspace), _ptr(d["view"]), _ptr(d["proj"]), _ptr(d["campos"]),
            _stream(dev)), "backward_window_cameras")
    return d


class _RasterizeWindow(torch.autograd.Function):
    """The autograd adapter of `window_forward` / `window_backward`: the V views of one optimisation window
    (train_gaussians.py:195-229) as ONE launch sequence.  Inputs: the shared rasterizer arguments, the list of per-view
    settings, then one `means2D` gradient carrier per view, then (viewmatrix, projmatrix, campos) of every view.
    Outputs: (color_0, depth_0, alpha_0, radii_0, color_1, ...).
    The backward runs once, when autograd has the output gradients of every view, and returns parameter gradients already
    summed over the views — and, when a camera tensor requires grad, that view's camera gradients from the same launch
    sequence (`window_backward(cameras=True)`).  `grad_fn.R`: the instances per view.

    `split_last`: the colour buffer of every view is handed out as TWO autograd outputs, channels [0, C-1) and channel
    C-1 — SplatLoc's `render` = image[:3] and `kp_prob` = image[-1] (gaussian_renderer/__init__.py:133-135) — so the
    outputs are (rgb_0, last_0, depth_0, alpha_0, radii_0, rgb_1, ...).  Their gradients then reach the kernel as
    separate planes (no zero-padded [C,H,W] copies and no add, which is what slicing one output costs in autograd),
    and a channel / auxiliary plane that did not reach the loss is skipped by the backward (color_refinement).
    `split_last` may also be an integer g in [1, C - 1): the outputs are then (image[:g], image[-1], ...) and the channels
    in between are not handed out at all (a wide [rgb | features | kp_score] table whose loss reads rgb and kp_score)."""

    @staticmethod
    def forward(ctx, means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, split_last, grad_span,
                forward_only, *rest):
        # rest: one means2D carrier per view, then (viewmatrix, projmatrix, campos) of every view — the settings' own tensors as
        # explicit autograd inputs, the way _RasterizeGaussians takes them (inputs 9-11 there), so that a pose parametrisation
        # upstream of them receives gradients
        V = len(settings)
        assert len(rest) in (V, 4 * V)
        # forward_only: no backward follows (_no_backward_follows, decided by the caller of apply); the render is told so
        f = window_forward(means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings,
                           forward_only=bool(forward_only))
        ctx.dev, ctx.P, ctx.st, ctx.R, ctx.tanfov = f.dev, f.P, f.st, f.R, f.tanfov
        ctx.head, ctx.grad_span = _split_head(split_last, f.st.channels), grad_span
        _save(ctx, f, [getattr(f, k) for k in _WINDOW_INPUTS], [t for cam in f.cams for t in cam] + [f.bg])
        outs = window_outputs(f, ctx.head)
        ctx.mark_non_differentiable(*(o[-1] for o in outs))
        ctx.set_materialize_grads(False)
        return tuple(t for o in outs for t in o)

    @staticmethod
    def backward(ctx, *gouts):
        inputs, buffers = _saved(ctx)
        n, V = len(_WINDOW_INPUTS), len(ctx.R)
        f = SimpleNamespace(dev=ctx.dev, P=ctx.P, V=V, st=ctx.st, R=ctx.R, tanfov=ctx.tanfov,
                            cams=[tuple(inputs[i:i + 3]) for i in range(n, len(inputs) - 1, 3)], bg=inputs[-1],
                            **dict(zip(_WINDOW_INPUTS, inputs)), **buffers)
        if ctx.head:
            grads = [gouts[5 * v:5 * v + 4] for v in range(V)]
        else:
            grads = [(gouts[4 * v], None, gouts[4 * v + 1], gouts[4 * v + 2]) for v in range(V)]
        # the joint call only when a camera tensor needs a gradient: otherwise the launch sequence is the plain one
        need = ctx.needs_input_grad[10 + V:]
        d = window_backward(f, grads, ctx.head, ctx.grad_span, cameras=any(need))
        # (means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, split_last, grad_span, forward_only,
        #  *means2D, *(viewmatrix, projmatrix, campos per view))
        cams = tuple(d[("view", "proj", "campos")[j % 3]][j // 3] if on else None for j, on in enumerate(need))
        return (d["m3"], d["col"], d["op"], d["sca"], d["rot"], d["cov"], None, None, None, None) + tuple(d["m2"][v] for v in range(V)) + cams


def rasterize_window(settings, means3D, means2D, colors_precomp, opacities, scales=None, rotations=None,
                     cov3D_precomp=None, split_last: bool = False, grad_span: Optional[list] = None):
    """`[GaussianRasterizer(s)(means3D, m2, opacities, colors_precomp=..., ...) for s, m2 in zip(settings, means2D)]`
    as one launch sequence per chunk of <= 8 views.  `settings`: GaussianRasterizationSettings per view (same
    image size / scale modifier / background); `means2D`: one gradient carrier per view.  Returns a list of
    (color, depth, alpha, radii) per view — bit-identical to the per-view calls; the backward sums the views'
    parameter gradients in-kernel (one gradient set per window instead of V sets + V accumulation passes).
    A view's `viewmatrix` / `projmatrix` / `campos` may require grad, as for the per-view call: the chunk's backward is then the
    joint one (`window_backward(cameras=True)`) and they receive their gradients (`campos`: zeros).
    `split_last`: (rgb [C-1,H,W], last [H,W], depth, alpha, radii) per view instead (an integer g: (image[:g], image[-1],
    ...)) — see _RasterizeWindow.
    `grad_span`: a list; every chunk's backward appends its gradient allocation (`window_grad_span`: flat, the pieces and a
    zeroed [2, P, 1] tail for the xyz_gradient_accum / denom increments) — the frame-parallel step reduces gradients and
    statistics as ONE in-place SUM (frame_parallel.reduce_step).
    An empty window (no settings) returns []."""
    settings, means2D = list(settings), list(means2D)
    if not settings and not means2D:
        return []
    if colors_precomp is None:
        raise Exception("rasterize_window needs precomputed colors (view-dependent SH colours: per-view calls)")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    if len(settings) != len(means2D) or not settings:
        raise Exception("rasterize_window: one means2D tensor per view")
    if not _window_compatible(settings):
        raise Exception("rasterize_window: the views of a window share image size, scale modifier and background")
    out = []
    # chunks of at most 8 views, and of at most 2^24 (view, Gaussian) rows: the kernels address rows with 24-bit multiplies
    # and the depth-order words keep the row in 24 bits (a scene of > 2 M Gaussians renders its window in smaller chunks)
    K = max(1, min(_native.MAX_WINDOW_VIEWS, (1 << 24) // max(int(means3D.shape[0]), 1)))
    for a in range(0, len(settings), K):
        cams = [t for rs in settings[a:a + K] for t in (rs.viewmatrix, rs.projmatrix, rs.campos)]
        forward_only = _no_backward_follows(means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp, *means2D[a:a + K], *cams)
        flat = _RasterizeWindow.apply(means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                      tuple(settings[a:a + K]), split_last, grad_span, forward_only, *means2D[a:a + K], *cams)
        n = 5 if _split_head(split_last, int(colors_precomp.shape[1])) else 4
        out += [tuple(flat[n * v:n * v + n]) for v in range(len(flat) // n)]
    return out


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Boolean mask of points in front of the near plane (view z > 0.2)."""
        lib = _native.load()
        _require_gpu(positions, "positions")
        rs = self.raster_settings
        dev = positions.device
        with torch.no_grad():
            pos = _prep(positions, dev)
            P = int(positions.shape[0])
            present = torch.zeros((P,), dtype=torch.uint8, device=dev)
            if P:
                view, proj = _prep(rs.viewmatrix, dev), _prep(rs.projmatrix, dev)
                with torch.cuda.device(dev):
                    _native.check(lib.splatraster_mark_visible(P, _ptr(pos), _ptr(view), _ptr(proj),
                                                               _ptr(present), _stream(dev)), "mark_visible")
        return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs)
