"""The two inner loops of SplatLoc as the rasterizer sees them, with the device-side pieces of this package in place
of the reference's chains of torch ops: drop-in bodies for `SplatLoc.color_refinement`'s iteration
(train_gaussians.py:272-297 — 26 000 of the ~35 000 rasterizer calls of a scene) and the learning-rate schedule it
calls.  `gaussians` is the reference's own GaussianModel object (or anything with the same attributes); its optimizer
may be torch.optim.Adam or splatloc_amd.optim.Adam (one launch over the 8 groups, key-primitive gate folded in).
"""
from __future__ import annotations

import os
import time

import math

import torch

from .densify import add_densification_stats_window
from .fused import render_window
from .losses import refinement_loss_and_grad


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000) -> float:
    """`helper` of gaussian_splatting/utils/general_utils.py:79-94 (the xyz learning-rate schedule)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    else:
        delay_rate = 1.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def update_learning_rate(gaussians, iteration) -> float:
    """GaussianModel.update_learning_rate (gaussian_model.py:311-326): the model's own method when it has one."""
    if hasattr(gaussians, "update_learning_rate"):
        return gaussians.update_learning_rate(iteration)
    for grp in gaussians.optimizer.param_groups:
        if grp["name"] == "xyz":
            grp["lr"] = expon_lr(iteration, lr_init=gaussians.lr_init, lr_final=gaussians.lr_final,
                                 lr_delay_mult=gaussians.lr_delay_mult, max_steps=gaussians.max_steps)
            return grp["lr"]
    return 0.0


def _direct_refine_ok(gaussians, pipe) -> bool:
    """SplatLoc's own configuration (SH degree 0, colours converted in Python, covariance in the rasterizer) on a non-empty
    model whose tensors all take gradients: the iteration can run without autograd (below)."""
    if not bool(pipe.convert_SHs_python) or bool(pipe.compute_cov3D_python) or int(gaussians.active_sh_degree) != 0:
        return False
    if int(gaussians._xyz.shape[0]) == 0 or not gaussians._xyz.is_cuda:
        return False
    return all(getattr(gaussians, a).requires_grad for a in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_kp_score",
                                                             "_scaling", "_rotation"))


RAW_BACKWARD = os.environ.get("SPLATLOC_RAW_BACKWARD", "1") != "0"     # (A/B and tests: 0 = the two-kernel chain)


def _raw_backward_ok(gaussians) -> bool:
    """The raw-parameter kernels cover SplatLoc's own layout: contiguous fp32 [P,3] log-scales, [P,4] quaternions, [P,1] logits,
    [P,1,3] SH dc, no higher SH coefficients, ONE key-point column (C = 4)."""
    if not RAW_BACKWARD:
        return False
    g = gaussians
    ok = lambda t, shp: (t.dtype is torch.float32 and t.is_contiguous() and tuple(t.shape[1:]) == shp and not (t.data_ptr() & 15))  # noqa: E731
    return (ok(g._scaling, (3,)) and ok(g._rotation, (4,)) and ok(g._opacity, (1,)) and ok(g._features_dc, (1, 3))
            and int(g._features_rest.shape[1]) == 0 and g._kp_score.dim() == 2 and ok(g._kp_score, (int(g._kp_score.shape[1]),))
            and int(g._kp_score.shape[1]) == 1)     # (C = 4: the accumulator rows' colour columns share the moments' 64-byte line)


_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_kp_score")


def _grads_direct(gaussians, settings, loss_grads, with_reg: bool, bounded=None):
    """The gradient part of a refinement iteration or a map step WITHOUT an autograd graph: the launch functions the graph
    path runs through its autograd Functions (fused.activate_forward / _backward, rasterizer.window_forward / _backward,
    losses.isotropic_forward), called directly.  At SplatLoc's frame size both steps are HOST-bound (tools/refine_idle.py,
    tools/hostprof_steps.py), and the autograd engine's hand-off of the backward nodes to its worker thread and its
    validation of the output gradients were a third of their host time.

        activations -> ONE window forward over `settings` -> loss_grads(outs) -> 0.01 * isotropic regulariser (with_reg)
        -> ONE window backward -> activation backward -> .grad

    With `_raw_backward_ok` the activations run inside the rasterizer's per-Gaussian kernels instead (raw-parameter mode
    of window_forward / window_backward: two launches and the activated-gradient tensors less, bit-identical values,
    tests/test_gpu_refine.py).  `outs`: (rgb, kp_prob, depth, opacity, radii) per view; `loss_grads` returns (loss,
    [(g_rgb, g_kp_prob, g_depth) per view]).  Gradients land in `.grad` exactly as autograd would leave them: `_xyz` <-
    dL/dmeans3D, `_features_rest` <- its empty gradient, `_kp_score` <- its gradient (a zero column when only RGB reaches
    the loss), `_marker` <- nothing.  `bounded`: window_forward's (the forward waits for no instance count).
    Returns (outs, loss, dL/dmeans2D [V, P, 3])."""
    from .fused import activate_backward, activate_forward
    from .losses import isotropic_forward
    from .rasterizer import window_backward, window_forward, window_outputs
    g = gaussians
    xyz = g._xyz
    raw = act = None
    if _raw_backward_ok(g):
        raw = (g._scaling.detach(), g._rotation.detach(), g._opacity.detach(), g._features_dc.detach(), g._kp_score.detach())
        frame = window_forward(xyz, None, None, None, None, None, settings, raw=raw, bounded=bounded)
    else:
        (scales, rotations, opacity, colors), act = activate_forward(xyz, g._features_dc, g._features_rest, g._scaling,
                                                                     g._rotation, g._opacity, g._kp_score, None, 0)
        frame = window_forward(xyz, colors, opacity, scales, rotations, None, settings, bounded=bounded)
    outs = window_outputs(frame, 3)
    loss, grads = loss_grads(outs)
    reg = None
    if with_reg:
        # 0.01 * isotropic regulariser on exp(_scaling) (train_gaussians.py:221-228): its gradient w.r.t. the ACTIVATED scales
        # joins the rasterizer's before the activation backward multiplies by exp(s)
        row_grad, out = isotropic_forward(frame.sca, g._marker.detach())
        reg = (row_grad, out, 0.01)
        loss = 0.01 * out[0] if loss is None else loss + 0.01 * out[0]
    d = window_backward(frame, [(g_rgb, g_kp, g_depth, None) for g_rgb, g_kp, g_depth in grads], 3, raw=raw, reg=reg)
    if raw is not None:
        fresh = (d["m3"], d["f_dc"], torch.empty_like(g._features_rest), d["scaling"], d["rotation"], d["opacity"], d["extra"])
    else:
        d_sca = d["sca"]
        if reg is not None:
            d_sca = d_sca + ((reg[2] * reg[1][1]) * reg[0]).view(-1, 1)
        _dx, d_fd, d_fr, d_sc, d_ro, d_op, d_ex = activate_backward(act, d_sca, d["rot"], d["op"], d["col"])
        fresh = (d["m3"], d_fd, d_fr, d_sc, d_ro, d_op, d_ex)
    for k, gr in zip(_PARAMS, fresh):
        if gr is not None:
            p = getattr(g, k)
            p.grad = gr if p.grad is None else p.grad + gr
    return outs, loss, d["m2"]


def _key_gate(gaussians, on: bool) -> None:
    """The key-primitive gate on xyz.grad (rows whose _marker exceeds 0.005 do not move): inside the fused Adam launch when
    the optimizer is splatloc_amd.optim.Adam, else the reference's masked assignment."""
    opt = gaussians.optimizer
    if hasattr(opt, "set_key_gate"):
        if on:
            opt.set_key_gate(gaussians._marker, 0.005)
        else:
            opt.set_key_gate(None)
    elif on and gaussians._xyz.grad is not None:
        gaussians._xyz.grad[gaussians._marker.detach().squeeze() > 0.005] = 0


def _color_refinement_step_direct(viewpoint_cam, gaussians, background, lambda_dssim, iteration, primitive_reg, bounded=None):
    """The iteration of `color_refinement_step` without an autograd graph (`_grads_direct`).  `bounded`: see `refine_bounded`."""
    from .fused import _view_settings

    def loss_grads(outs):
        rgb = outs[0][0]
        gt_image = viewpoint_cam.original_image
        if gt_image.device != rgb.device:
            gt_image = gt_image.to(rgb.device)
        loss, g_image = refinement_loss_and_grad(rgb, gt_image, lambda_dssim)
        return loss, [(g_image, None, None)]

    with torch.no_grad():
        outs, loss, _m2 = _grads_direct(gaussians, [_view_settings(viewpoint_cam, gaussians, background, 1.0)], loss_grads, False,
                                        bounded=bounded)
        radii = outs[0][4]
        opt = gaussians.optimizer
        _key_gate(gaussians, primitive_reg)
        if hasattr(opt, "set_radii_update") and radii.dtype == torch.int32 and radii.is_contiguous():
            opt.set_radii_update(radii, gaussians.max_radii2D)      # the statistics line rides the fused Adam launch
        else:
            add_densification_stats_window(None, [radii], None, None, gaussians.max_radii2D)
        opt.step()
        opt.zero_grad(set_to_none=True)
        update_learning_rate(gaussians, iteration)
    return loss


def color_refinement_step(viewpoint_cam, gaussians, pipe, background, lambda_dssim: float, iteration: int,
                          primitive_reg: bool = True, render_path: str = "auto"):
    """One iteration of SplatLoc.color_refinement (train_gaussians.py:275-297):

        render -> (1 - l) L1 + l (1 - SSIM) on the RGB channels -> backward -> key-primitive gate on xyz.grad ->
        max_radii2D update -> optimizer.step -> zero_grad -> update_learning_rate(iteration)

    with: ONE window-of-one launch sequence whose `render` / `kp_prob` / depth / opacity are separate autograd outputs —
    only `render` reaches the loss, so the backward kernel runs on 3 colour channels without the depth / alpha terms
    and no zero-padded gradient images are built; the fused L1 + SSIM loss (two kernels instead of five grouped 11x11
    convolutions and their autograd backward); the `max_radii2D` line as one launch without boolean-mask indexing
    (the reference: two `nonzero` + a device->host sync); the gate inside the fused Adam launch when the optimizer is
    splatloc_amd.optim.Adam (else the reference's masked assignment).  Returns the loss tensor (no host sync).
    `render_path`: "auto" (graph-free when the configuration allows it), "window" (the window-of-one under autograd) or
    "per-view" (the drop-in `render()` -> `diff_gauss.GaussianRasterizer` call an unmodified train_gaussians.py issues)."""
    if render_path not in ("auto", "window", "per-view"):
        raise ValueError(f"color_refinement_step: unknown render_path {render_path!r}")
    if render_path == "auto" and _direct_refine_ok(gaussians, pipe):
        return _color_refinement_step_direct(viewpoint_cam, gaussians, background, lambda_dssim, iteration, primitive_reg)
    if render_path == "per-view":
        from .fused import render
        pkg = render(viewpoint_cam, gaussians, pipe, background)
    else:
        pkg = render_window([viewpoint_cam], gaussians, pipe, background, batched=True)[0][0]
    if pkg is None:
        return None
    image, radii = pkg["render"], pkg["radii"]
    gt_image = viewpoint_cam.original_image.to(image.device)
    loss, g_image = refinement_loss_and_grad(image, gt_image, lambda_dssim)   # the fused launch holds the gradient: no loss node
    image.backward(g_image)
    opt = gaussians.optimizer
    with torch.no_grad():
        _key_gate(gaussians, primitive_reg)
        add_densification_stats_window(None, [radii], None, None, gaussians.max_radii2D)
        opt.step()
        opt.zero_grad(set_to_none=True)
        update_learning_rate(gaussians, iteration)
    return loss


def _bounded_refine_ok(gaussians, pipe, viewpoints, background) -> bool:
    """`refine_bounded` applies: the graph-free iteration (`_direct_refine_ok`), the fused Adam with its gate and its radii line,
    and frames the binned front end renders (the bounded forward's scope: include/splatraster.h)."""
    from . import _native
    from .fused import _view_settings
    from .rasterizer import _window_compatible
    opt = gaussians.optimizer
    if not viewpoints or not _direct_refine_ok(gaussians, pipe) or not (hasattr(opt, "set_gate") and hasattr(opt, "set_radii_update")):
        return False
    distinct = list({id(vp): vp for vp in viewpoints}.values())
    if not _window_compatible([_view_settings(vp, gaussians, background, 1.0) for vp in distinct]):
        return False
    vp = viewpoints[0]
    return _native.bounded_supported(int(gaussians._xyz.shape[0]), 1, int(vp.image_width), int(vp.image_height))


def _host_optimizer_state(opt) -> list:
    """What an Adam step changes on the HOST: every group's learning rate and every parameter's step count."""
    return [(grp["lr"], [float(opt.state[p]["step"]) if opt.state.get(p) else None for p in grp["params"]])
            for grp in opt.param_groups]


def _restore_host_optimizer_state(opt, snap) -> None:
    for grp, (lr, steps) in zip(opt.param_groups, snap):
        grp["lr"] = lr
        for p, stp in zip(grp["params"], steps):
            st = opt.state.get(p)
            if st:      # (a state created by a gated step holds zero moments — what the first real step creates)
                st["step"].fill_(0.0 if stp is None else stp)


def refine_bounded(viewpoints, gaussians, pipe, background, lambda_dssim: float, first_iteration: int, n_iterations: int,
                   primitive_reg: bool = True, initial_capacity=None) -> dict:
    """`n_iterations` iterations of `color_refinement_step` (iteration numbers first_iteration, first_iteration + 1, ...; iteration
    i renders viewpoints[i % len(viewpoints)]) whose forwards do not stop the host for the instance count: every iteration's
    launches — bounded forward, loss, backward, gated Adam — are enqueued without a wait, so the host runs ahead of the device.

    The frame is rendered into ONE reusable binning buffer of `capacity` instances (rasterizer.BoundedWindow).  Capacity policy:
    `initial_capacity`, or 1.25 x the R of one ordinary (synchronous) forward of viewpoints[0], at least 4096; after an overflow
    1.5 x the R that did not fit.  After enqueuing an iteration the loop reads the status block's host mirror (no
    synchronisation).  A frame that does not fit sets the block's STICKY overflow flag on the device: from that sequence on every
    forward renders background and every Adam launch returns at once, so no parameter, moment or max_radii2D changes behind
    it.  When the host sees the flag it synchronises once, grows the buffer, clears the block, restores the host-side step counts
    and learning rates of iteration `first_tag`, and resumes there — the replay is exact, and the end state is that of the
    plain loop (bit for bit in the library's deterministic mode).

    Falls back to the loop of `color_refinement_step` calls where the mode does not apply (`_bounded_refine_ok`).
    Returns {"losses": [loss tensor per iteration], "rewinds": int, "capacity_history": [capacities used], "bounded": bool,
    "enqueue_seconds": host time until the last iteration was enqueued (replays included; the final wait is not)}."""
    from .fused import _view_settings
    from .rasterizer import BoundedWindow, window_forward
    t_start = t_enqueued = time.perf_counter()
    viewpoints = list(viewpoints)
    n_iterations = int(n_iterations)
    if n_iterations <= 0 or not _bounded_refine_ok(gaussians, pipe, viewpoints, background):
        losses = [color_refinement_step(viewpoints[i % len(viewpoints)], gaussians, pipe, background, lambda_dssim,
                                        first_iteration + i, primitive_reg=primitive_reg) for i in range(n_iterations)]
        return {"losses": losses, "rewinds": 0, "capacity_history": [], "bounded": False, "enqueue_seconds": time.perf_counter() - t_start}
    dev = gaussians._xyz.device
    opt = gaussians.optimizer
    if initial_capacity is None:
        with torch.no_grad():     # one ordinary forward: its count is this loop's only host wait when every frame fits
            g = gaussians
            if _raw_backward_ok(g):
                raw = (g._scaling.detach(), g._rotation.detach(), g._opacity.detach(), g._features_dc.detach(), g._kp_score.detach())
                probe = window_forward(g._xyz, None, None, None, None, None, [_view_settings(viewpoints[0], g, background, 1.0)], raw=raw)
            else:
                from .fused import activate_forward
                (sca, rot, opa, col), _act = activate_forward(g._xyz, g._features_dc, g._features_rest, g._scaling, g._rotation,
                                                              g._opacity, g._kp_score, None, 0)
                probe = window_forward(g._xyz, col, opa, sca, rot, None, [_view_settings(viewpoints[0], g, background, 1.0)])
        capacity = max(4096, int(math.ceil(1.25 * sum(probe.R))))
        del probe
    else:
        capacity = int(initial_capacity)
    bw = BoundedWindow(dev, capacity)
    history = [capacity]
    losses, snaps, rewinds = [], {}, 0
    opt.set_gate(bw.status)
    try:
        i = 0
        while True:
            if i < n_iterations:
                snaps[i] = _host_optimizer_state(opt)
                bw.next_tag = i
                losses.append(_color_refinement_step_direct(viewpoints[i % len(viewpoints)], gaussians, background, lambda_dssim,
                                                            first_iteration + i, primitive_reg, bounded=bw))
                i += 1
                # ONE read of the mirror, never a wait.  It copies last_tag BEFORE overflow: the sequences in front of
                # `last_tag` have finished — their stores are all visible — so a clear flag read after it proves that none
                # of them overflowed, and their snapshots can go.  (The sequence `last_tag` itself may still raise the flag.)
                rec = bw.status.read()
                if not rec.overflow:
                    for k in [k for k in snaps if k < int(rec.last_tag)]:
                        del snaps[k]
                    continue
            else:
                t_enqueued = time.perf_counter()
            # the flag was seen, or everything is enqueued: ONE wait, and only the record read BEHIND it is acted on — a flag
            # seen in front of it is a hint (the mirror may lag the stream)
            torch.cuda.synchronize(dev)
            rec = bw.status.read()
            if not rec.overflow:
                if i >= n_iterations:
                    break
                continue
            k, need = int(rec.first_tag), int(rec.first_total)
            if k not in snaps or need <= capacity:
                raise RuntimeError(f"refine_bounded: inconsistent overflow record (tag {k}, total {need}, capacity {capacity})")
            capacity = max(int(math.ceil(1.5 * need)), capacity + 1)
            bw.capacity = capacity
            history.append(capacity)
            rewinds += 1
            bw.status.clear()      # (the stream is idle: the mirror reads clear from here on)
            _restore_host_optimizer_state(opt, snaps[k])
            del losses[k:]
            for j in [j for j in snaps if j > k]:
                del snaps[j]
            i = k
    finally:
        opt.set_gate(None)
        torch.cuda.synchronize(dev)
        bw.close()
    return {"losses": losses, "rewinds": rewinds, "capacity_history": history, "bounded": True,
            "enqueue_seconds": t_enqueued - t_start}


def _cameras_require_grad(settings) -> bool:
    return any(t is not None and t.requires_grad for rs in settings for t in (rs.viewmatrix, rs.projmatrix, rs.campos))


def _map_grads_direct(mine, gaussians, pipe, background, config, with_reg: bool):
    """The gradient part of `map_step` without an autograd graph (`_grads_direct`; the per-view losses already carry their
    gradients).  Leaves the raw-parameter gradients in `.grad`.  Returns (pkgs, loss, [dL/dmeans2D per view]) or None when the
    configuration needs the general path (view-dependent colours, python covariance, mixed image sizes, an empty model)."""
    from .fused import _view_settings
    from .losses import mapping_loss_window
    from .rasterizer import _window_compatible
    from . import _native
    if not _direct_refine_ok(gaussians, pipe) or len(mine) > _native.MAX_WINDOW_VIEWS:
        return None
    if int(gaussians._xyz.shape[0]) * len(mine) > (1 << 24):          # (rasterize_window would chunk the window: general path)
        return None
    settings = [_view_settings(vp, gaussians, background, 1.0) for vp in mine]
    if not _window_compatible(settings):
        return None
    if _cameras_require_grad(settings):       # key-frame poses optimised with the map: the autograd window path (joint backward)
        return None
    pkgs = []

    def loss_grads(outs):
        for rgb, kp, depth, alpha, radii in outs:
            pkgs.append({"render": rgb, "kp_prob": kp, "depth": depth, "opacity": alpha, "radii": radii})
        _t, g, loss = mapping_loss_window(config, pkgs, mine)      # g = [g_render, g_depth, g_kp] per view
        return loss, [(g[3 * v], g[3 * v + 2], g[3 * v + 1]) for v in range(len(mine))]

    with torch.no_grad():
        _outs, loss, m2 = _grads_direct(gaussians, settings, loss_grads, with_reg)
    return pkgs, loss, [m2[v] for v in range(len(mine))]


# how a multi-GPU map_step sums its payload: "ring" (one all-reduce) or "rs_ag" (reduce-scatter + all-gather);
# frame_parallel.reduce_step(mode=...).  bench.py --reduce sets it; every rank must use the same value
REDUCE_MODE = os.environ.get("SPLATLOC_REDUCE_MODE", "ring")
# what the last multi-GPU map_step exchanged (frame_parallel.reduce_step's info: collectives, path, bytes) — monitoring
LAST_STEP_INFO: dict = {}


def map_step(viewpoints, gaussians, pipe, background, config, iteration_count: int, *, densify=None,
             gaussian_reset: int = 0, seed: int = 0, group=None, render_path: str = "auto", distributed: bool = True):
    """One iteration of the loop body of SplatLoc.map (train_gaussians.py:188-267) on the window `viewpoints` (the
    caller has drawn it: `all_viewpoint_stack[torch.randperm(len(...))[:window_size]]`, :195), with the device-side
    pieces of this package, single- or multi-GPU:

        render the window + per-view get_loss_mapping + get_loss_marker      -> fused.render_window (ONE launch sequence)
        + 0.01 * isotropic regulariser (primitive_reg)                        -> losses.isotropic_loss (no .cpu() mask)
        backward                                                              -> one window backward (gradients summed in-kernel)
        key-primitive gate, max_radii2D / add_densification_stats per view    -> one statistics launch
        densify_and_prune every `densify["every"]` iterations (offset)        -> densify.densify_and_prune
        reset_opacity_nonvisible every `gaussian_reset` iterations            -> densify.reset_opacity_nonvisible
        optimizer.step, zero_grad, update_learning_rate(iteration_count)

    Frame-parallel data parallelism (torch.distributed initialised, one process per GPU, a full replica of
    the scene per rank): the views of the window are dealt round-robin to the ranks (frame_parallel.shard_views); ONE SUM
    all-reduce carries the parameter gradients and the statistics increments, ONE MAX all-reduce max_radii2D and (on a
    reset step) the visibility union — two collectives per step (frame_parallel.reduce_step; a rank without views, world
    size > window size, contributes zeros) —, so every replica takes the SAME optimizer step and densifies identically (the split noise is
    counter-based: keyed by (seed, iteration_count, source row, copy)) — the replicas stay bit-identical without ever
    broadcasting parameters.  The regulariser is added on rank 0 only (the reduced gradient contains it once).
    `densify`: dict(grad_threshold, min_opacity, extent, size_threshold, every, offset) or None.
    `render_path`: "auto" (the graph-free window path when the configuration allows it, else the window path under autograd),
    "window" (always under autograd) or "per-view" (the reference's loop of per-view render() calls through the drop-in
    autograd.Function — what an unmodified train_gaussians.py issues); LAST_STEP_INFO["render_path"] says which one ran.
    Returns the rank's loss tensor (None on a rank without work)."""
    import torch.distributed as dist
    from .densify import densify_and_prune, reset_opacity_nonvisible
    from .frame_parallel import collectives_active, reduce_step, shard_views
    from .losses import isotropic_loss, mapping_loss_window
    # `distributed=False`: this rank reconstructs its OWN scene although a process group exists (one scene per GPU,
    # /root/reference/replica.sh; bench.py --stage scene --replicas): no collective at all.  (A group of ONE rank exchanges
    # nothing either, unless SPLATLOC_FORCE_COLLECTIVES=1 asks for the collectives anyway: the one-GPU RCCL contact test.)
    multi = distributed and collectives_active(group)
    rank = dist.get_rank(group) if multi else 0
    world = dist.get_world_size(group) if multi else 1
    primitive_reg = bool(config["Training"].get("primitive_reg", True))
    viewpoints = list(viewpoints)
    mine = [viewpoints[i] for i in shard_views(list(range(len(viewpoints))), rank, world)]
    if render_path not in ("auto", "window", "per-view"):
        raise ValueError(f"map_step: unknown render_path {render_path!r}")
    if multi and world > 1 and any(getattr(vp, a, None) is not None and getattr(vp, a).requires_grad for vp in viewpoints
                                   for a in ("world_view_transform", "full_proj_transform", "camera_center")):
        raise NotImplementedError("map_step: camera tensors that require grad on more than one rank (no pose exchange)")
    direct = None
    if mine and render_path == "auto":
        direct = _map_grads_direct(mine, gaussians, pipe, background, config, primitive_reg and rank == 0)
    ran = "direct-window" if direct is not None else ("per-view" if render_path == "per-view" else "window")
    if direct is not None:
        pkgs, loss, grads2d_direct = direct
    else:
        grads2d_direct = None
        per_view = render_path == "per-view"        # the literal loop: one render() per view, each with its own activations
        pkgs, _ = render_window(mine, gaussians, pipe, background, batched=not per_view, share_activations=not per_view)
        pairs = [(p, v) for p, v in zip(pkgs, mine) if p is not None]      # views and packages filtered TOGETHER
        pkgs, mine = [p for p, _ in pairs], [v for _, v in pairs]
        # the per-view losses carry their own gradients (one fused launch each): ONE backward on the rasterizer's outputs, no
        # per-view loss nodes / gradient scalings / additions (losses.mapping_loss_window)
        tensors, grads, loss = mapping_loss_window(config, pkgs, mine)
        if primitive_reg and rank == 0 and gaussians._xyz.shape[0] > 0:
            reg = 0.01 * isotropic_loss(torch.exp(gaussians._scaling), gaussians._marker)
            tensors, grads = tensors + [reg], grads + [None]
            loss = reg.detach() if loss is None else loss + reg.detach()
        if tensors:
            torch.autograd.backward(tensors, grads)
    params = [getattr(gaussians, a) for a in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_kp_score", "_scaling",
                                              "_rotation")]      # `_marker` never receives a gradient in map()
    opt = gaussians.optimizer
    with torch.no_grad():
        P = int(gaussians._xyz.shape[0])
        dev = gaussians._xyz.device
        grads2d = grads2d_direct if grads2d_direct is not None else [p["viewspace_points"].grad for p in pkgs]
        radii = [p["radii"] for p in pkgs]
        update_gaussian = bool(densify) and iteration_count % int(densify["every"]) == int(densify.get("offset", 0))
        reset_now = bool(gaussian_reset) and iteration_count % gaussian_reset == 0 and not update_gaussian
        seen = None
        if reset_now:       # the union of the window's visibility masks (gaussian_model.py:384-392)
            seen = torch.zeros(P, dtype=torch.float32, device=dev)
            for p in pkgs:
                seen = torch.maximum(seen, (p["radii"] > 0).to(torch.float32))      # visibility_filter = radii > 0
        if multi:
            # everything the replicas exchange in this step, in TWO collectives (frame_parallel.reduce_step):
            #   SUM over [parameter gradients | increments of xyz_gradient_accum, denom]
            #   MAX over [max_radii2D | visibility flags of a reset step]
            for p in params:        # a rank without views: zero gradients (incl. the empty `_features_rest` group, so that
                if p.grad is None:  # every replica's optimizer creates the same state)
                    p.grad = torch.zeros_like(p)
            live = [p for p in params if p.numel()]
            inc = torch.zeros((2, P, 1), device=dev)
            if pkgs:
                add_densification_stats_window(grads2d, radii, inc[0], inc[1], gaussians.max_radii2D)
            g_out, inc_out, info = reduce_step([p.grad for p in live], sum_extras=[inc[0], inc[1]],
                                               max_extras=[gaussians.max_radii2D] + ([seen] if seen is not None else []),
                                               group=group, mode=REDUCE_MODE, force=True)
            for p, g in zip(live, g_out):
                p.grad = g          # views of the reduced buffer: no copy back
            gaussians.xyz_gradient_accum += inc_out[0]
            gaussians.denom += inc_out[1]
            LAST_STEP_INFO.clear()
            LAST_STEP_INFO.update(info)
        else:
            LAST_STEP_INFO.clear()
            if pkgs:
                add_densification_stats_window(grads2d, radii, gaussians.xyz_gradient_accum, gaussians.denom, gaussians.max_radii2D)
        LAST_STEP_INFO["render_path"] = ran
        _key_gate(gaussians, primitive_reg)
        if update_gaussian:
            densify_and_prune(gaussians, densify["grad_threshold"], densify["min_opacity"], densify["extent"],
                              densify["size_threshold"], seed=seed, draw_id=iteration_count)
        if reset_now:
            reset_opacity_nonvisible(gaussians, [seen > 0])
        opt.step()
        opt.zero_grad(set_to_none=True)
        update_learning_rate(gaussians, iteration_count)
    return loss
