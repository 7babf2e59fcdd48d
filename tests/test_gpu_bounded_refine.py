"""training.refine_bounded and the gated Adam launch (splatraster_adam_step[_radii]_gated) — needs an MI355X.

The bounded loop enqueues every iteration without waiting for the frame's instance count; a frame that does not fit its buffer
gates every later Adam launch on the device, and the host replays from that iteration with a larger buffer.  In the library's
deterministic mode the loop must therefore end in EXACTLY the state of the plain loop of `color_refinement_step` calls — every
parameter, both moments, the step counts, the learning rates, max_radii2D and every loss, bit for bit — with and without replays."""
import types

import pytest
import torch

from splatloc_amd import _native
from splatloc_amd.camera import PinholeCamera
from splatloc_amd.optim import Adam as FusedAdam
from splatloc_amd.rasterizer import BoundedWindow, window_forward
from splatloc_amd.synthetic import make_scene
from splatloc_amd.fused import _view_settings
from splatloc_amd.training import color_refinement_step, refine_bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, P = 64, 48, 2000
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "marker", "kp_score", "scaling", "rotation")
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "marker": "_marker",
        "kp_score": "_kp_score", "scaling": "_scaling", "rotation": "_rotation"}
LR = {"xyz": 1.6e-4 * 6.0, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 5e-2, "marker": 5e-2, "kp_score": 5e-2,
      "scaling": 1e-3 * 6.0, "rotation": 1e-3}
PIPE = types.SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False)
ZOOM = (1.6, 1.3, 1.0, 1.15)     # camera 0 sees the fewest Gaussians, camera 2 the most


def _model():
    """SplatLoc's GaussianModel attributes over a seeded scene; identical every call"""
    dev = torch.device(DEV)
    sc = make_scene(P, W, H, 4, 31, scale_median=0.03)
    g = torch.Generator().manual_seed(11)
    par = lambda t: torch.nn.Parameter(t.to(dev).contiguous().requires_grad_(True))  # noqa: E731
    pc = types.SimpleNamespace(
        _xyz=par(sc.means3D.clone()), _features_dc=par(((sc.features[:, :3] - 0.5) / 0.28209479177387814)[:, None, :].contiguous()),
        _features_rest=par(torch.zeros(P, 0, 3)), _opacity=par(torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))),
        _marker=par((torch.rand(P, 1, generator=g) < 0.05).float() * torch.rand(P, 1, generator=g) * 0.9),
        _kp_score=par(torch.rand(P, 1, generator=g)), _scaling=par(torch.log(sc.scales)), _rotation=par(sc.rotations.clone()),
        active_sh_degree=0, max_sh_degree=0, lr_init=1.6e-4 * 6.0, lr_final=1.6e-6 * 6.0, lr_delay_mult=0.01, max_steps=30000)
    pc.optimizer = FusedAdam([{"params": [getattr(pc, ATTR[k])], "lr": LR[k], "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    pc.max_radii2D = torch.zeros(P, device=dev)
    return pc


def _cameras():
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(12)
    cams = []
    for k, zoom in enumerate(ZOOM):
        ang = torch.tensor(0.02 * (k - 2))
        R = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]])
        cam = PinholeCamera(W, H, zoom * W / 2.0, zoom * W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, R, torch.tensor([0.01 * k, 0.0, 0.0])).to(dev)
        cam.original_image = torch.rand(3, H, W, generator=g).to(dev)
        cams.append(cam)
    return cams


def _count(pc, cam, bg):
    """R of the existing forward"""
    with torch.no_grad():
        raw = (pc._scaling.detach(), pc._rotation.detach(), pc._opacity.detach(), pc._features_dc.detach(), pc._kp_score.detach())
        return sum(window_forward(pc._xyz, None, None, None, None, None, [_view_settings(cam, pc, bg, 1.0)], raw=raw).R)


def _state(pc):
    out = {"max_radii2D": pc.max_radii2D.clone()}
    for grp in pc.optimizer.param_groups:
        k, p = grp["name"], grp["params"][0]
        out["param " + k] = p.detach().clone()
        out["lr " + k] = grp["lr"]
        st = pc.optimizer.state.get(p)
        out["has state " + k] = bool(st)
        if st:
            out["step " + k] = float(st["step"])
            out["exp_avg " + k], out["exp_avg_sq " + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


def _assert_state_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            bits = torch.int32 if a[k].dtype == torch.float32 else a[k].dtype
            assert torch.equal(a[k].view(bits), b[k].view(bits)), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.fixture(scope="module")
def reference():
    """10 iterations of the existing loop from the seeded start, in deterministic mode: run once, never modified"""
    _native.set_deterministic(True)
    try:
        pc, cams = _model(), _cameras()
        bg = torch.zeros(3, device=DEV)
        counts = [_count(pc, c, bg) for c in cams]
        losses = [color_refinement_step(cams[i % 4], pc, PIPE, bg, 0.2, 1 + i) for i in range(10)]
        torch.cuda.synchronize()
        return {"state": _state(pc), "losses": [x.clone() for x in losses], "counts": counts}
    finally:
        _native.set_deterministic(False)


def _run_bounded(initial_capacity):
    _native.set_deterministic(True)
    try:
        pc, cams = _model(), _cameras()
        res = refine_bounded(cams, pc, PIPE, torch.zeros(3, device=DEV), 0.2, 1, 10, initial_capacity=initial_capacity)
        torch.cuda.synchronize()
        return pc, res
    finally:
        _native.set_deterministic(False)


def test_loop_with_rewinds_ends_in_the_plain_loops_state(reference):
    counts = reference["counts"]
    assert counts[2] > counts[0] > 0, counts
    pc, res = _run_bounded(counts[0])
    assert res["bounded"]
    print("rewinds", res["rewinds"], "capacity_history", res["capacity_history"], "counts", counts)
    assert 1 <= res["rewinds"] <= 4          # at most one per distinct camera
    hist = res["capacity_history"]
    assert hist[0] == counts[0] and all(b > a for a, b in zip(hist, hist[1:])) and len(hist) == res["rewinds"] + 1
    _assert_state_equal(_state(pc), reference["state"])
    assert len(res["losses"]) == 10
    for i, (a, b) in enumerate(zip(res["losses"], reference["losses"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"loss of iteration {i}"
    assert pc.optimizer._gate is None        # the gate is the loop's, not the optimizer's


def test_loop_without_rewind_ends_in_the_plain_loops_state(reference):
    pc, res = _run_bounded(None)
    assert res["bounded"] and res["rewinds"] == 0 and len(res["capacity_history"]) == 1
    assert res["capacity_history"][0] == max(4096, -(-5 * reference["counts"][0] // 4))
    _assert_state_equal(_state(pc), reference["state"])
    for i, (a, b) in enumerate(zip(res["losses"], reference["losses"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"loss of iteration {i}"


def _adam_case(misaligned):
    """two optimizers over identical parameters, gradients and (non-trivial) moments, a radii line each.  `misaligned`: the xyz
    parameter starts 4 bytes behind a 16-byte boundary, so the launch is the scalar kernel (adam_kernel) and not the 16-byte form
    (adam_quad_kernel)"""
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(3)
    shapes = {"xyz": (777, 3), "opacity": (777, 1), "rotation": (777, 4)}
    base = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    grads = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    gate = (torch.rand(777, 1, generator=g) * 0.01).to(dev)
    radii = torch.randint(0, 9, (777,), generator=g, dtype=torch.int32).to(dev)
    out = []
    for _ in range(2):
        params = {k: torch.nn.Parameter(v.clone().to(dev)) for k, v in base.items()}
        if misaligned:
            buf = torch.empty(777 * 3 + 1, device=dev)
            buf[1:].copy_(base["xyz"].reshape(-1))
            params["xyz"] = torch.nn.Parameter(buf[1:].view(777, 3))
        assert (params["xyz"].data_ptr() % 16 != 0) == misaligned and params["xyz"].is_contiguous()
        opt = FusedAdam([{"params": [params[k]], "lr": 1e-2, "name": k} for k in shapes], lr=0.0, eps=1e-15)
        opt.set_key_gate(gate, 0.005)
        max_r = torch.full((777,), 2.0, device=dev)
        for _step in range(2):      # two plain steps: moments and step counts beyond their initial values
            for k in shapes:
                params[k].grad = grads[k].to(dev)
            opt.step()
        for k in shapes:
            params[k].grad = (0.5 * grads[k]).to(dev)
        opt.set_radii_update(radii, max_r)
        out.append((params, opt, max_r))
    return out


def _adam_state(params, opt, max_r):
    out = {"max_radii2D": max_r.clone()}
    for k, p in params.items():
        out["param " + k] = p.detach().clone()
        out["exp_avg " + k], out["exp_avg_sq " + k] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
    return out


@pytest.mark.parametrize("misaligned", [False, True])
def test_gated_adam_is_the_plain_step_or_nothing(misaligned):
    dev = torch.device(DEV)
    (pa, oa, ra), (pb, ob, rb) = _adam_case(misaligned)
    before = _adam_state(pb, ob, rb)
    # a status block whose overflow flag is set: one bounded forward into a buffer of capacity 0
    sc = make_scene(300, W, H, 4, 5, scale_median=0.08)
    cam = sc.camera.to(dev)
    from splatloc_amd import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, cam.world_view_transform,
                                       cam.full_proj_transform, 0, cam.camera_center, False, False)
    bw = BoundedWindow(dev, 0)
    window_forward(sc.means3D.to(dev), sc.features.to(dev), sc.opacities.to(dev), sc.scales.to(dev), sc.rotations.to(dev), None,
                   [rs], bounded=bw)
    torch.cuda.synchronize()
    assert bw.status.read().overflow == 1
    ob.set_gate(bw.status)
    ob.step()                              # gated, flag set: nothing moves (the radii line neither)
    torch.cuda.synchronize()
    _assert_state_equal(_adam_state(pb, ob, rb), before)
    assert float(ob.state[pb["xyz"]]["step"]) == 3.0       # the host-side count advanced: the loop that owns the block rewinds it
    # flag clear: the gated step from the same state == the ungated step
    bw.status.clear()
    for p in pb.values():
        ob.state[p]["step"].fill_(2.0)
    oa_radii, _ = oa._radii_update         # (the gated step consumed ob's request: the same radii again)
    ob.set_radii_update(oa_radii, rb)
    ob.step()
    oa.step()
    torch.cuda.synchronize()
    _assert_state_equal(_adam_state(pb, ob, rb), _adam_state(pa, oa, ra))
    assert not torch.equal(before["param xyz"], pb["xyz"].detach()) and not torch.equal(before["max_radii2D"], rb)
    bw.close()
