"""Pose parameterisations and a pose-refinement loop on the rasterizer's pose gradients.

The reference ships `utils/optimization_utils.py` (axis-angle / quaternion / 6-D rotation + translation -> 4x4 transform) for
optimising a camera pose through the renderer, but nothing in the reference calls it and its rasterizer returns no gradient
for the camera: the path ends at `viewmatrix`.  Here it continues — `diff_gauss.GaussianRasterizer` returns
dL/dviewmatrix, dL/dprojmatrix and dL/dcampos when those tensors require a gradient (tests/test_gpu_pose.py) —
so the helpers have a use.  Same names, argument meaning and return shapes as utils/optimization_utils.py:5-66, restated
without pytorch3d (not installed here); the rotation conversions follow the published formulas pytorch3d implements
(quaternions real part first; 6-D rotations: Zhou et al., "On the Continuity of Rotation Representations", rows b1, b2, b1 x b2).

Two deliberate differences, both where the reference is broken:
  * `axis_angle_to_matrix` of the ZERO vector is the identity here (the reference divides by |w| = 0 and returns NaN —
    its own "TODO: Identity would cause the problem", optimization_utils.py:4); gradients at zero are those of the
    first-order expansion R = I + [w]x;
  * `six_t_to_transform_matrix` returns the matrix (the reference's last line is a bare `return`, :66: it returns None).

Host-side torch code: these are 3x3 / 4x4 operations per camera, not a kernel.
"""
from __future__ import annotations

import torch


def _skew(v: torch.Tensor) -> torch.Tensor:
    z = torch.zeros_like(v[..., 0])
    return torch.stack([torch.stack([z, -v[..., 2], v[..., 1]], dim=-1),
                        torch.stack([v[..., 2], z, -v[..., 0]], dim=-1),
                        torch.stack([-v[..., 1], v[..., 0], z], dim=-1)], dim=-2)


def axis_angle_to_matrix(data: torch.Tensor) -> torch.Tensor:
    """Rodrigues: [..., 3] axis * angle -> [..., 3, 3] (optimization_utils.py:5-22).  R = I + sin(t) K + (1 - cos(t)) K^2 with
    K = [w / t]x, written as I + a [w]x + b [w]x^2 with a = sin(t) / t, b = (1 - cos(t)) / t^2 so that t -> 0 is regular."""
    t2 = (data * data).sum(dim=-1, keepdim=True)
    small = t2 < 1e-12
    t2s = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(t2s)
    a = torch.where(small, 1.0 - t2 / 6.0, torch.sin(t) / t)[..., None]
    b = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(t)) / t2s)[..., None]
    W = _skew(data)
    eye = torch.eye(3, dtype=data.dtype, device=data.device).expand(*data.shape[:-1], 3, 3)
    return eye + a * W + b * (W @ W)


def quaternion_to_matrix(q: torch.Tensor) -> torch.Tensor:
    """[..., 4] quaternion (real part first, any non-zero norm) -> [..., 3, 3]."""
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return o.reshape(q.shape[:-1] + (3, 3))


def matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] rotation -> [..., 4] unit quaternion, real part first and non-negative.  The candidate with the largest
    of (1 + trace, 1 + 2 R_ii - trace) is used: its square root is >= 1/2, so no component is divided by a small number."""
    m = R.reshape(R.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    q_abs2 = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], dim=-1)
    q_abs = torch.sqrt(q_abs2.clamp_min(0.0))
    cand = torch.stack([
        torch.stack([q_abs2[..., 0], m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs2[..., 1], m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs2[..., 2], m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs2[..., 3]], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = q_abs.argmax(dim=-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    return torch.where(q[..., :1] < 0, -q, q)


def quaternion_to_axis_angle(q: torch.Tensor) -> torch.Tensor:
    """[..., 4] unit quaternion (real part first) -> [..., 3] axis * angle, angle in [0, pi] for a non-negative real part."""
    n = torch.linalg.norm(q[..., 1:], dim=-1, keepdim=True)
    r = q[..., :1]
    small = n < 1e-6
    rs = torch.where(small, r.clamp_min(1e-6), torch.ones_like(r))
    x2 = (n / rs) ** 2
    # angle / |v| = 2 atan2(|v|, r) / |v|; for |v| -> 0: (2 / r) (1 - (|v| / r)^2 / 3)
    scale = torch.where(small, (2.0 / rs) * (1.0 - x2 / 3.0), 2.0 * torch.atan2(n, r) / torch.where(small, torch.ones_like(n), n))
    return q[..., 1:] * scale


def matrix_to_axis_angle(rot: torch.Tensor) -> torch.Tensor:
    """[N, 3, 3] -> [N, 3] (optimization_utils.py:24-29)."""
    return quaternion_to_axis_angle(matrix_to_quaternion(rot))


def rotation_6d_to_matrix(d6: torch.Tensor) -> torch.Tensor:
    """[..., 6] -> [..., 3, 3]: Gram-Schmidt of the two 3-vectors; ROWS b1, b2, b1 x b2."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def _transform(R: torch.Tensor, trans: torch.Tensor) -> torch.Tensor:
    bs = R.shape[0]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=R.dtype, device=R.device).expand(bs, 1, 4)
    return torch.cat([torch.cat([R, trans[:, :, None]], dim=2), bottom], dim=1)


def at_to_transform_matrix(rot: torch.Tensor, trans: torch.Tensor) -> torch.Tensor:
    """axis-angle [bs, 3] + translation [bs, 3] -> [bs, 4, 4] (optimization_utils.py:31-42)."""
    return _transform(axis_angle_to_matrix(rot), trans)


def qt_to_transform_matrix(rot: torch.Tensor, trans: torch.Tensor) -> torch.Tensor:
    """quaternion [bs, 4] (real part first) + translation [bs, 3] -> [bs, 4, 4] (optimization_utils.py:44-54)."""
    return _transform(quaternion_to_matrix(rot), trans)


def six_t_to_transform_matrix(rot: torch.Tensor, trans: torch.Tensor) -> torch.Tensor:
    """6-D rotation [bs, 6] + translation [bs, 3] -> [bs, 4, 4] (optimization_utils.py:55-66; see the module header)."""
    return _transform(rotation_6d_to_matrix(rot), trans)


def camera_tensors(W2C: torch.Tensor, projection_matrix: torch.Tensor):
    """(world_view_transform, full_proj_transform, camera_center) as differentiable functions of a [4, 4] world-to-camera
    matrix — utils/camera_utils.py:129-139: the row-vector (transposed) view matrix, view @ projection, and the camera centre
    -R^T t (the reference inverts the 4x4; for a rigid transform that is the same point, without the LU)."""
    view = W2C.transpose(0, 1)
    proj = view @ projection_matrix
    campos = -(W2C[:3, :3].transpose(0, 1) @ W2C[:3, 3])
    return view, proj, campos


def refine_pose(render_target, gaussians: dict, camera, W2C_init: torch.Tensor, iterations: int = 100, lr_rot: float = 2e-3,
                lr_trans: float = 3e-3, depth_weight: float = 0.2, background: torch.Tensor | None = None, on_step=None,
                graph_free: bool = True):
    """Gradient descent on a camera pose through the rasterizer: the pose is W2C = T(w, t) @ W2C_init with an axis-angle w
    and a translation t (both start at zero), the loss is L1(colour) + depth_weight * L1(depth) against `render_target` =
    (colour [C,H,W], depth [1,H,W] or None), Adam on (w, t).  `gaussians`: dict(means3D, colors, opacities, scales, rotations)
    of device tensors (activated values, as the rasterizer takes them); `camera`: intrinsics holder with image_width / height,
    tanfovx / tanfovy and `projection_matrix` (splatloc_amd.camera.PinholeCamera or the reference's Camera).
    Returns (W2C [4,4] detached, history of loss values as one device tensor [iterations]).

    `graph_free` (default): an iteration is ONE launch sequence with no torch operator in it — the rasterizer's launch functions
    called directly (rasterizer.view_forward / view_backward, no autograd graph), `splatraster_l1_rgbd_loss` for the loss and
    its gradient planes, `splatraster_pose_step` for the chain rule to (w, t), the Adam step and the next camera tensors
    (csrc/pose.hip): no autograd graph, no torch.optim, the 6 numbers never visit the host.  `graph_free=False` is round
    4's loop (autograd through the 4x4 algebra + torch.optim.Adam): the same iterates to float32 rounding
    (tests/test_gpu_pose.py), ~3x the host time per iteration."""
    if not graph_free:
        return _refine_pose_autograd(render_target, gaussians, camera, W2C_init, iterations, lr_rot, lr_trans, depth_weight,
                                     background, on_step)
    import ctypes as C
    from . import _native
    from ._host import _stream
    from .rasterizer import GaussianRasterizationSettings, view_backward, view_forward
    lib = _native.load()
    dev = gaussians["means3D"].device
    tgt_c, tgt_d = render_target
    tgt_c = tgt_c.to(dev).float().contiguous()
    tgt_d = None if (tgt_d is None or not depth_weight) else tgt_d.to(dev).float().contiguous()
    W2C0 = W2C_init.to(dev).float().contiguous()
    Pm = camera.projection_matrix.to(dev).float().contiguous()
    H, W = int(camera.image_height), int(camera.image_width)
    bg = background if background is not None else torch.zeros(int(tgt_c.shape[0]) if tgt_c.shape[0] <= 3 else 0, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    state = torch.zeros(20, **f32)          # w, t, Adam moments, step (splatraster_pose_step)
    view, proj, campos = torch.empty(4, 4, **f32), torch.empty(4, 4, **f32), torch.empty(3, **f32)
    hist = torch.zeros(iterations, **f32)
    g_color, g_depth = torch.empty_like(tgt_c), torch.empty((1, H, W), **f32)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    b1, b2, eps = 0.9, 0.999, 1e-8          # torch.optim.Adam's defaults, as round 4's loop used them

    def step(advance, grads=(None, None, None)):
        _native.check(lib.splatraster_pose_step(ptr(grads[0]), ptr(grads[1]), ptr(grads[2]), ptr(W2C0), ptr(Pm), lr_rot, lr_trans,
                                                b1, b2, eps, advance, ptr(state), ptr(view), ptr(proj), ptr(campos), _stream(dev)),
                      "pose_step")

    step(0)
    rs = GaussianRasterizationSettings(H, W, camera.tanfovx, camera.tanfovy, bg, 1.0, view, proj, 0, campos, False, False)
    n_c, n_d = tgt_c.numel(), H * W
    with torch.no_grad():
        for it in range(iterations):
            f = view_forward(gaussians["means3D"], None, gaussians["colors"], gaussians["opacities"], gaussians["scales"],
                             gaussians["rotations"], None, rs, view, proj, campos)
            _native.check(lib.splatraster_l1_rgbd_loss(n_c, ptr(f.color), ptr(tgt_c), n_d, ptr(f.depth), ptr(tgt_d), float(depth_weight),
                                                       ptr(g_color), ptr(g_depth), C.c_void_p(hist.data_ptr() + 4 * it),
                                                       _stream(dev)), "l1_rgbd_loss")
            d = view_backward(f, g_color, g_depth if tgt_d is not None else None, None, want_pose=True)
            del f       # (the frame's buffers go back to the allocator before the next forward takes its own)
            step(1, (d["view"], d["proj"], d["campos"]))
            if on_step:
                on_step(it, hist[it])
        w, t = state[:3].clone()[None], state[3:6].clone()[None]
        return (at_to_transform_matrix(w, t)[0] @ W2C0).detach(), hist


def window_chunk(P: int, window: int = 8) -> int:
    """Frames per launch sequence of `refine_poses`: min(window, 8, 2**24 // P) and at least 1 — `rasterize_window`'s rule (the
    kernels address the (view, Gaussian) rows of a window with 24-bit multiplies)."""
    from . import _native
    return max(1, min(int(window), _native.MAX_WINDOW_VIEWS, (1 << 24) // max(int(P), 1)))


def _check_refine_poses(render_targets, gaussians, camera, W2C_init, iterations, window):
    """Argument errors of `refine_poses` (shapes only: nothing here reads a tensor's data or touches a device).  Returns
    (N, colour, depth or None)."""
    try:
        tgt_c, tgt_d = render_targets
    except (TypeError, ValueError):
        raise ValueError("refine_poses: render_targets is (colour [N,C,H,W], depth [N,1,H,W] or None)") from None
    if not isinstance(tgt_c, torch.Tensor) or tgt_c.dim() != 4:
        raise ValueError("refine_poses: the colour target is one [N,C,H,W] tensor")
    N, Cn, H, W = (int(x) for x in tgt_c.shape)
    if N == 0:
        raise ValueError("refine_poses: no frames (N == 0)")
    if (H, W) != (int(camera.image_height), int(camera.image_width)):
        raise ValueError(f"refine_poses: targets are {H}x{W}, the camera {int(camera.image_height)}x{int(camera.image_width)}")
    if Cn != int(gaussians["colors"].shape[1]):
        raise ValueError(f"refine_poses: {Cn} target channels, {int(gaussians['colors'].shape[1])} colour columns")
    if isinstance(tgt_d, (list, tuple)):     # per-frame depth targets: all of them or none
        if len(tgt_d) != N or any(d is None for d in tgt_d) != all(d is None for d in tgt_d):
            raise ValueError("refine_poses: a depth target for some frames only (give one for every frame, or None)")
        if tgt_d[0] is not None and any(int(d.numel()) != H * W for d in tgt_d):
            raise ValueError(f"refine_poses: every depth target is [1,{H},{W}]")
        tgt_d = None if tgt_d[0] is None else torch.stack([d.reshape(1, H, W) for d in tgt_d])
    if tgt_d is not None:
        if tgt_d.dim() != 4 or int(tgt_d.shape[0]) != N:
            raise ValueError(f"refine_poses: depth targets for {int(tgt_d.shape[0]) if tgt_d.dim() else 0} of {N} frames "
                             "(give one for every frame, or None)")
        if tuple(tgt_d.shape[1:]) != (1, H, W):
            raise ValueError(f"refine_poses: the depth target is [N,1,{H},{W}], not {tuple(tgt_d.shape)}")
    if not isinstance(W2C_init, torch.Tensor) or tuple(W2C_init.shape) != (N, 4, 4):
        raise ValueError(f"refine_poses: W2C_init is [{N},4,4], one start pose per frame")
    if int(iterations) < 0 or int(window) < 1:
        raise ValueError("refine_poses: iterations >= 0 and window >= 1")
    return N, tgt_c, tgt_d


def refine_poses(render_targets, gaussians: dict, camera, W2C_init: torch.Tensor, iterations: int = 100, lr_rot: float = 2e-3,
                 lr_trans: float = 3e-3, depth_weight: float = 0.2, background: torch.Tensor | None = None, window: int = 8):
    """`refine_pose` (graph-free) for N query frames of one camera model against one frozen map, `window` frames per launch
    sequence: render_targets = (colour [N,C,H,W], depth [N,1,H,W] or None), W2C_init [N,4,4].  The frames are taken in chunks
    of K = `window_chunk(P, window)`; a chunk runs its own `iterations` iterations, each ONE launch sequence whose length
    does not depend on K: rasterizer.window_forward -> splatraster_l1_rgbd_loss_window -> rasterizer.window_backward_cameras
    (camera gradients of the K views, nothing per Gaussian: the map is frozen) -> splatraster_pose_step_window (one thread per
    frame; every frame keeps its own Adam state).  No torch operator, no autograd graph, no host read of a gradient inside an
    iteration.  Returns (W2C [N,4,4], loss history [iterations, N] on the device).  Argument errors — shape mismatches, N == 0, a
    depth target for some frames only — raise ValueError before any device access."""
    N, tgt_c, tgt_d = _check_refine_poses(render_targets, gaussians, camera, W2C_init, iterations, window)
    import ctypes as C
    from . import _native
    from ._host import _stream
    from .rasterizer import GaussianRasterizationSettings, window_backward_cameras, window_forward
    lib = _native.load()
    dev = gaussians["means3D"].device
    tgt_c = tgt_c.to(dev).float().contiguous()
    tgt_d = None if (tgt_d is None or not depth_weight) else tgt_d.to(dev).float().contiguous()
    W2C0 = W2C_init.to(dev).float().contiguous()
    Pm = camera.projection_matrix.to(dev).float().contiguous()
    H, W, Cn = int(camera.image_height), int(camera.image_width), int(tgt_c.shape[1])
    bg = background if background is not None else torch.zeros(Cn if Cn <= 3 else 0, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    hist = torch.zeros((iterations, N), **f32)
    out = torch.empty((N, 4, 4), **f32)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    b1, b2, eps = 0.9, 0.999, 1e-8          # torch.optim.Adam's defaults, as refine_pose
    n_c, n_d = Cn * H * W, H * W
    K = window_chunk(int(gaussians["means3D"].shape[0]), window)
    with torch.no_grad():
        for a in range(0, N, K):
            k = min(K, N - a)
            state = torch.zeros((k, 20), **f32)     # per frame: w, t, Adam moments, step (splatraster_pose_step)
            view, proj = torch.empty((k, 4, 4), **f32), torch.empty((k, 4, 4), **f32)
            d = {"view": torch.empty((k, 4, 4), **f32), "proj": torch.empty((k, 4, 4), **f32), "campos": torch.empty((k, 3), **f32)}
            ws = torch.empty((lib.splatraster_window_camera_workspace_bytes(k),), dtype=torch.uint8, device=dev)
            g_color, g_depth = torch.empty((k, Cn, H, W), **f32), torch.empty((k, 1, H, W), **f32)

            def step(advance):      # (no campos: precomputed colours do not read the camera centre)
                _native.check(lib.splatraster_pose_step_window(
                    k, ptr(d["view"]), ptr(d["proj"]), None, ptr(W2C0[a:a + k]), ptr(Pm), lr_rot, lr_trans, b1, b2, eps, advance,
                    ptr(state), ptr(view), ptr(proj), None, _stream(dev)), "pose_step_window")

            step(0)
            # the camera tensors of frame j are rows of `view` / `proj`, rewritten in place by every step
            settings = [GaussianRasterizationSettings(H, W, camera.tanfovx, camera.tanfovy, bg, 1.0, view[j], proj[j], 0, None,
                                                      False, False) for j in range(k)]
            grads = [(g_color[j], g_depth[j] if tgt_d is not None else None, None) for j in range(k)]
            lv = (_native.L1View * k)()
            for j in range(k):
                lv[j].target_color = tgt_c[a + j].data_ptr()
                lv[j].target_depth = None if tgt_d is None else tgt_d[a + j].data_ptr()
                lv[j].g_color, lv[j].g_depth = g_color[j].data_ptr(), g_depth[j].data_ptr()
            for it in range(iterations):
                f = window_forward(gaussians["means3D"], gaussians["colors"], gaussians["opacities"], gaussians["scales"],
                                   gaussians["rotations"], None, settings)
                for j in range(k):
                    lv[j].color, lv[j].depth = f.color[j].data_ptr(), f.depth[j].data_ptr()
                _native.check(lib.splatraster_l1_rgbd_loss_window(k, lv, n_c, n_d, float(depth_weight),
                                                                  C.c_void_p(hist.data_ptr() + 4 * (it * N + a)), _stream(dev)),
                              "l1_rgbd_loss_window")
                window_backward_cameras(f, grads, ws, d)
                del f       # (the window's buffers go back to the allocator before the next forward takes its own)
                step(1)
            out[a:a + k] = at_to_transform_matrix(state[:, :3], state[:, 3:6]) @ W2C0[a:a + k]
        return out, hist


class WindowPoses:
    """Key-frame poses optimised TOGETHER with the map over a window (the trainer SplatLoc's `map()` descends from does this;
    SplatLoc dropped it because its data sets come with poses): the device-side optimiser of N world-to-camera matrices on top of
    `splatraster_pose_step_window` — frame j is W2C_j = T(w_j, t_j) @ W2C_init[j] with an axis-angle w_j and a translation t_j
    (both start at zero) and its own Adam moments, `refine_poses`' parametrisation and defaults.

    `view` [N,4,4], `proj` [N,4,4] and `campos` [N,3] hold the camera tensors of all frames as three LEAF tensors that require
    grad; `cameras(ids)` hands out their rows (views: put them into a viewpoint's world_view_transform / full_proj_transform /
    camera_center, or into GaussianRasterizationSettings), so a backward through `rasterize_window` — the joint window backward,
    `rasterizer.window_backward(cameras=True)` — leaves every frame's gradient in the rows of `.grad`.  `step(ids)` advances the
    listed frames from those rows (one launch per <= 8 frames: chain rule to (w, t), Adam, the next camera tensors written in
    place — the 6 numbers of a frame never visit the host) and zeroes the rows; a frame's result does not depend on its slot or
    on the frames stepped with it.  `fixed`: frames that no step moves — the gauge of a joint optimisation is free unless one
    pose (or the map's positions) is held.  `W2C()`: the current poses [N,4,4]."""

    def __init__(self, W2C_init: torch.Tensor, projection_matrix: torch.Tensor, lr_rot: float = 2e-3, lr_trans: float = 3e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, fixed=()):
        if not isinstance(W2C_init, torch.Tensor) or W2C_init.dim() != 3 or tuple(W2C_init.shape[1:]) != (4, 4) or not W2C_init.shape[0]:
            raise ValueError("WindowPoses: W2C_init is [N,4,4] with N >= 1, one start pose per frame")
        if tuple(projection_matrix.shape) != (4, 4):
            raise ValueError("WindowPoses: projection_matrix is [4,4]")
        N = int(W2C_init.shape[0])
        self.fixed = frozenset(int(i) for i in fixed)
        if any(i < 0 or i >= N for i in self.fixed):
            raise ValueError(f"WindowPoses: fixed frames outside 0 .. {N - 1}")
        if not W2C_init.is_cuda:
            raise RuntimeError("WindowPoses runs on the GPU: W2C_init is on " + str(W2C_init.device))
        dev = W2C_init.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.N, self.dev = N, dev
        self.lr_rot, self.lr_trans, self.betas, self.eps = float(lr_rot), float(lr_trans), (float(betas[0]), float(betas[1])), float(eps)
        self.W2C0 = W2C_init.detach().to(**f32).contiguous()
        self.Pm = projection_matrix.detach().to(**f32).contiguous()
        self.state = torch.zeros((N, 20), **f32)        # per frame: w, t, Adam moments, step (splatraster_pose_step)
        self.view = torch.empty((N, 4, 4), **f32).requires_grad_(True)
        self.proj = torch.empty((N, 4, 4), **f32).requires_grad_(True)
        self.campos = torch.empty((N, 3), **f32).requires_grad_(True)
        for a in range(0, N, 8):
            self._launch(a, min(8, N - a), 0, None, self.state, self.view, self.proj, self.campos, self.W2C0)

    def _launch(self, a, k, advance, grads, state, view, proj, campos, W2C0):
        """splatraster_pose_step_window on rows [a, a + k) of the given tensors (`grads`: (dview, dproj, dcampos or None), the
        same rows)"""
        import ctypes as C
        from . import _native
        from ._host import _stream
        row = lambda t: None if t is None else C.c_void_p(t.data_ptr() + a * t.stride(0) * 4)  # noqa: E731
        gv, gp, gc = grads if grads is not None else (None, None, None)
        _native.check(_native.load().splatraster_pose_step_window(
            k, row(gv), row(gp), row(gc), row(W2C0), C.c_void_p(self.Pm.data_ptr()), self.lr_rot, self.lr_trans, self.betas[0],
            self.betas[1], self.eps, advance, row(state), row(view), row(proj), row(campos), _stream(self.dev)), "pose_step_window")

    def cameras(self, ids):
        """(viewmatrix, projmatrix, campos) of frame `ids` (an int), or a list of such triples: rows of the three leaves"""
        if isinstance(ids, int):
            return self.view[ids], self.proj[ids], self.campos[ids]
        return [(self.view[int(i)], self.proj[int(i)], self.campos[int(i)]) for i in ids]

    def W2C(self) -> torch.Tensor:
        with torch.no_grad():
            return at_to_transform_matrix(self.state[:, :3], self.state[:, 3:6]) @ self.W2C0

    def zero_grad(self, ids=None) -> None:
        for t in (self.view, self.proj, self.campos):
            if t.grad is not None:
                if ids is None:
                    t.grad.zero_()
                else:
                    t.grad[ids] = 0.0

    def step(self, ids) -> None:
        """One Adam step of the frames `ids` (any order, no repeats) from the rows of view.grad / proj.grad / campos.grad, which
        are then zeroed; `fixed` frames are skipped.  A tensor without .grad contributes zeros."""
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids) or any(i < 0 or i >= self.N for i in ids):
            raise ValueError(f"WindowPoses.step: ids are distinct frames in 0 .. {self.N - 1}")
        move = [i for i in ids if i not in self.fixed]
        with torch.no_grad():
            gv = self.view.grad if self.view.grad is not None else torch.zeros_like(self.view)
            gp = self.proj.grad if self.proj.grad is not None else torch.zeros_like(self.proj)
            gc = self.campos.grad
            for a in range(0, len(move), 8):
                chunk = move[a:a + 8]
                k = len(chunk)
                if chunk == list(range(chunk[0], chunk[0] + k)):     # neighbouring rows: the kernel works on them where they are
                    self._launch(chunk[0], k, 1, (gv, gp, gc), self.state, self.view, self.proj, self.campos, self.W2C0)
                    continue
                sel = torch.tensor(chunk, device=self.dev)
                state, view, proj, campos = self.state[sel], self.view[sel], self.proj[sel], self.campos[sel]
                self._launch(0, k, 1, (gv[sel], gp[sel], None if gc is None else gc[sel]), state, view, proj, campos, self.W2C0[sel])
                self.state[sel] = state
                self.view.data[sel], self.proj.data[sel], self.campos.data[sel] = view, proj, campos
            if ids:
                self.zero_grad(torch.tensor(ids, device=self.dev))


def _refine_pose_autograd(render_target, gaussians: dict, camera, W2C_init: torch.Tensor, iterations: int = 100,
                          lr_rot: float = 2e-3, lr_trans: float = 3e-3, depth_weight: float = 0.2,
                          background: torch.Tensor | None = None, on_step=None):
    """round 4's refine_pose: autograd through the pose algebra and the drop-in autograd.Function, torch.optim.Adam."""
    from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    dev = gaussians["means3D"].device
    tgt_c, tgt_d = render_target
    W2C0 = W2C_init.to(dev).float()
    P = camera.projection_matrix.to(dev)
    bg = background if background is not None else torch.zeros(int(tgt_c.shape[0]) if tgt_c.shape[0] <= 3 else 0, device=dev)
    w = torch.zeros(1, 3, device=dev, requires_grad=True)
    t = torch.zeros(1, 3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([{"params": [w], "lr": lr_rot}, {"params": [t], "lr": lr_trans}])
    carrier = torch.zeros_like(gaussians["means3D"])
    hist = torch.zeros(iterations, device=dev)
    for it in range(iterations):
        W2C = at_to_transform_matrix(w, t)[0] @ W2C0
        view, proj, campos = camera_tensors(W2C, P)
        rs = GaussianRasterizationSettings(int(camera.image_height), int(camera.image_width), camera.tanfovx, camera.tanfovy,
                                           bg, 1.0, view, proj, 0, campos, False, False)
        color, depth, _alpha, _radii = GaussianRasterizer(raster_settings=rs)(
            means3D=gaussians["means3D"], means2D=carrier, shs=None, colors_precomp=gaussians["colors"],
            opacities=gaussians["opacities"], scales=gaussians["scales"], rotations=gaussians["rotations"], cov3D_precomp=None)
        loss = (color - tgt_c).abs().mean()
        if tgt_d is not None and depth_weight:
            loss = loss + depth_weight * (depth - tgt_d).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        hist[it] = loss.detach()
        if on_step:
            on_step(it, loss)
    with torch.no_grad():
        return (at_to_transform_matrix(w, t)[0] @ W2C0).detach(), hist
