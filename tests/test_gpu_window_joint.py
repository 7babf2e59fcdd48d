"""The joint backward of a window on the GPU (splatraster_backward_window_joint, csrc/window_joint_bwd.hip): parameter gradients
summed over the views AND the camera gradients of every view from one compositing backward — against the CPU oracle, against the
two window calls that existed before it (rasterizer.window_backward / window_backward_cameras) on the same frame, at the kernel's
block / set / ticket edges, under autograd (rasterize_window with camera tensors that require grad), pose.WindowPoses, and key-frame
poses optimised together with the map end to end.

Bars: camera gradients TOL (test_gpu_pose.py / test_gpu_pose_window.py), parameter gradients and dL/dmeans2D assert_grad_close's
defaults (test_gpu_window.py outside its strict mode).  Cameras and output gradients are built as test_gpu_pose_window.py builds
them."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from splatloc_amd.camera import PinholeCamera
from splatloc_amd.synthetic import make_scene
from tests.helpers import assert_grad_close, oracle_backward, oracle_forward

pytestmark = pytest.mark.gpu

TOL = dict(rtol=3e-3, atol_scale=3e-4)      # test_gpu_pose.py test_pose_gradients_match_oracle
PARAMS = ("m3", "col", "op", "sca", "rot", "cov")
ORACLE = {"m3": "dL_dmeans3D", "col": "dL_dcolors", "op": "dL_dopacities", "sca": "dL_dscales", "rot": "dL_drotations"}


def _rot(ax, ay):
    cx, sx, cy, sy = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float32)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float32)
    return Ry @ Rx


def _cameras(W, H):
    """eight distinct cameras: rotated and translated by different small amounts, four different (tanfovx, tanfovy)"""
    f = W / 2.0
    spec = [(f, f, 0.00, 0.15, (0.05, -0.03, 0.20)), (1.15 * f, 0.9 * f, 0.04, -0.10, (-0.04, 0.02, 0.10)),
            (f, f, -0.03, 0.05, (0.02, 0.04, -0.05)), (0.85 * f, 1.1 * f, 0.02, 0.08, (0.00, -0.05, 0.15)),
            (f, f, 0.05, -0.04, (0.06, 0.00, 0.05)), (1.05 * f, 1.05 * f, -0.05, -0.12, (-0.02, -0.02, 0.25)),
            (f, f, 0.01, 0.11, (0.03, 0.03, 0.00)), (f, f, -0.02, -0.07, (-0.05, 0.01, 0.12))]
    return [PinholeCamera(W, H, fx, fy, (W - 1) / 2.0 + 0.4, (H - 1) / 2.0 - 0.2, _rot(ax, ay), torch.tensor(t))
            for fx, fy, ax, ay, t in spec]


def _out_grads(n, Cn, H, W, seed, bare=(1,)):
    """random dL/dout per view; the views in `bare` have no depth and no alpha gradient (NULL planes)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for v in range(n):
        gc, gd, ga = ((2.0 * torch.rand(c, H, W, generator=g) - 1.0) / (H * W) for c in (Cn, 1, 1))
        out.append((gc, None, None) if v in bare else (gc, gd, ga))
    return out


def _oracle(sc, cam, grads):
    """the oracle's backward of one view: camera gradients, parameter gradients, dL/dmeans2D, R"""
    gc, gd, ga = grads
    s = dataclasses.replace(sc, camera=cam, dL_dcolor=gc, dL_ddepth=gd, dL_dalpha=ga)
    f = oracle_forward(s)
    b = oracle_backward(f, s, use_depth=gd is not None, use_alpha=ga is not None)
    out = {"view": b["dL_dviewmatrix"], "proj": b["dL_dprojmatrix"], "R": int(f["num_rendered"]), "m2": b["dL_dmeans2D"]}
    out.update({k: np.asarray(b[name], dtype=np.float64) for k, name in ORACLE.items()})
    return out


def _settings(sc, cams, dev):
    from splatloc_amd import GaussianRasterizationSettings
    bg = sc.bg.to(dev)
    return [GaussianRasterizationSettings(c.image_height, c.image_width, c.tanfovx, c.tanfovy, bg, 1.0,
                                          c.world_view_transform.to(dev), c.full_proj_transform.to(dev), 0, c.camera_center.to(dev),
                                          False, False) for c in cams]


def _dev():
    return torch.device("cuda:0")


def _frame(sc, cams, cov=None):
    from splatloc_amd import rasterizer as R
    dev = _dev()
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    if cov is None:
        return R.window_forward(t(sc.means3D), t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations), None,
                                _settings(sc, cams, dev))
    return R.window_forward(t(sc.means3D), t(sc.features), t(sc.opacities), None, None, t(cov), _settings(sc, cams, dev))


def _np(d):
    return {k: (None if v is None else v.detach().cpu().numpy()) for k, v in d.items() if k not in ("flat", "tail")}


def _joint(f, grads):
    """the call under test: rasterizer.window_backward(cameras=True) on the frame `f`"""
    from splatloc_amd import rasterizer as R
    dev = _dev()
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    d = R.window_backward(f, [(t(gc), None, t(gd), t(ga)) for gc, gd, ga in grads], cameras=True)
    torch.cuda.synchronize()
    V = f.V
    assert d["view"].shape == (V, 4, 4) and d["proj"].shape == (V, 4, 4) and d["campos"].shape == (V, 3) and d["m2"].shape == (V, f.P, 3)
    return _np(d)


def _two_calls(f, grads):
    """the reference on the same frame: window_backward, then window_backward_cameras (both older than the joint call)"""
    from splatloc_amd import rasterizer as R
    dev = _dev()
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    d = R.window_backward(f, [(t(gc), None, t(gd), t(ga)) for gc, gd, ga in grads])
    assert "view" not in d
    c = R.window_backward_cameras(f, [tuple(t(g) for g in gs) for gs in grads])
    torch.cuda.synchronize()
    return {**_np(d), **_np(c)}


def _check_cams(name, d, v, ref, rv=None, nonzero=True):
    """view v of `d` against `ref` ([4,4] arrays, or [V,4,4] arrays indexed by rv)"""
    rview, rproj = (ref["view"], ref["proj"]) if rv is None else (ref["view"][rv], ref["proj"][rv])
    if nonzero:
        assert float(np.abs(rview).max()) > 0 and float(np.abs(rproj).max()) > 0     # cannot pass on zeros
    assert_grad_close(f"{name} dL_dviewmatrix[{v}]", d["view"][v], rview, **TOL)
    assert_grad_close(f"{name} dL_dprojmatrix[{v}]", d["proj"][v], rproj, **TOL)
    assert not d["campos"].any()


def _check_params(name, d, ref, m2=True):
    n = 0
    for k in PARAMS:
        if ref.get(k) is None:
            assert d.get(k) is None, k
            continue
        assert float(np.abs(ref[k]).max()) > 0, k
        assert_grad_close(f"{name} {k}", d[k], np.asarray(ref[k]).reshape(d[k].shape))
        n += 1
    assert n >= 4
    if m2:
        for v in range(d["m2"].shape[0]):
            assert_grad_close(f"{name} means2D[{v}]", d["m2"][v], ref["m2"][v])


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene8():
    sc = make_scene(3000, 160, 96, 4, 70, scale_median=0.03)
    cams = _cameras(160, 96)
    grads = _out_grads(8, 4, 96, 160, 11)
    return sc, cams, grads, [_oracle(sc, c, g) for c, g in zip(cams, grads)]


def _oracle_sum(ref, views):
    out = {k: sum(ref[v][k] for v in views) for k in ORACLE}
    out["m2"] = [ref[v]["m2"] for v in views]
    return out


@pytest.mark.parametrize("V", [1, 2, 3, 8])
def test_joint_matches_the_oracle(scene8, V):
    sc, cams, grads, ref = scene8
    f = _frame(sc, cams[:V])
    assert f.R == [r["R"] for r in ref[:V]]
    d = _joint(f, grads[:V])
    for v in range(V):
        _check_cams(f"V={V}", d, v, ref[v])
    _check_params(f"V={V}", d, _oracle_sum(ref, range(V)))


# ---- 2. against the two existing window calls on one frame -----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [
    dict(P=6000, W=320, H=240, C=4, seed=401, scale_median=0.03, V=5),     # SplatLoc's window: 5 views, [rgb | kp]
    dict(P=3000, W=333, H=201, C=35, seed=402, scale_median=0.03, V=3),    # shared colour rows, the TQ = 1 tail, a ragged frame
    dict(P=2000, W=160, H=96, C=40, seed=403, scale_median=0.04, V=2),     # a tail of eight columns: TQ = 4
    dict(P=2500, W=160, H=96, C=7, seed=404, scale_median=0.04, V=2),      # generic C: the gather over the per-view rows
])
def test_joint_matches_the_two_window_calls(cfg):
    cfg = dict(cfg)
    V = cfg.pop("V")
    sc = make_scene(**cfg)
    cams = _cameras(cfg["W"], cfg["H"])[:V]
    grads = _out_grads(V, cfg["C"], cfg["H"], cfg["W"], 21)
    f = _frame(sc, cams)
    assert all(r > 0 for r in f.R)
    ref, d = _two_calls(f, grads), _joint(f, grads)
    _check_params(str(cfg["C"]), d, ref)
    for v in range(V):
        _check_cams(str(cfg["C"]), d, v, ref, rv=v)


def test_joint_cov3d_precomp_with_a_colour_only_loss():
    sc = make_scene(2500, 256, 192, 4, 407, scale_median=0.03)
    g = torch.Generator().manual_seed(5)
    Lm = torch.randn(2500, 3, 3, generator=g) * 0.03
    S = Lm @ Lm.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
    cams = _cameras(256, 192)[:4]
    grads = _out_grads(4, 4, 192, 256, 22, bare=(0, 1, 2, 3))             # no depth, no alpha gradient in any view
    f = _frame(sc, cams, cov=cov)
    ref, d = _two_calls(f, grads), _joint(f, grads)
    assert d["sca"] is None and d["rot"] is None and d["cov"].shape == (2500, 6)
    _check_params("cov", d, ref)
    for v in range(4):
        _check_cams("cov", d, v, ref, rv=v)


# ---- 3. block, set and ticket edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 4353])
def test_block_set_and_ticket_edges(P):
    """one thread, one short of / exactly / one past a block, and 17 blocks + 1 Gaussian: more blocks than the 16 sets, so
    blockIdx % POSE_SETS wraps and two sets take two tickets; no Gaussians at all"""
    sc = make_scene(P, 64, 48, 4, 300 + P % 7, scale_median=0.05)
    if P == 1:      # the one Gaussian in front of all three cameras
        sc.means3D = torch.tensor([[0.1, -0.05, 2.0]])
    cams = _cameras(64, 48)[:3]
    grads = _out_grads(3, 4, 48, 64, 12)
    f = _frame(sc, cams)
    d = _joint(f, grads)
    if P == 0:
        assert f.R == [0, 0, 0] and not d["view"].any() and not d["proj"].any() and not d["campos"].any()
        assert d["m3"].shape == (0, 3) and d["m2"].shape == (3, 0, 3)
        return
    ref = [_oracle(sc, c, g) for c, g in zip(cams, grads)]
    for v in range(3):
        assert f.R[v] == ref[v]["R"] and ref[v]["R"] > 0
        _check_cams(f"P={P}", d, v, ref[v])
    _check_params(f"P={P} oracle", d, _oracle_sum(ref, range(3)))
    _check_params(f"P={P} window", d, _two_calls(f, grads))


# ---- 4. a view that sees nothing ---------------------------------------------------------------------------------------------------

def test_a_view_that_sees_nothing():
    sc = make_scene(2000, 128, 96, 4, 41, scale_median=0.04)
    cams = _cameras(128, 96)[:3]
    cams[1] = PinholeCamera(128, 96, 64.0, 64.0, 63.9, 47.3, torch.diag(torch.tensor([-1.0, 1.0, -1.0])), torch.tensor([0.02, 0.0, 0.1]))
    grads = _out_grads(3, 4, 96, 128, 13, bare=())
    f = _frame(sc, cams)
    assert f.R[1] == 0 and f.R[0] > 0 and f.R[2] > 0
    d = _joint(f, grads)
    assert not d["view"][1].any() and not d["proj"][1].any() and not d["campos"][1].any()       # all 35, exactly
    assert not d["m2"][1].any()
    # the window without that view, through the two older calls
    f2 = _frame(sc, [cams[0], cams[2]])
    ref = _two_calls(f2, [grads[0], grads[2]])
    _check_params("without the blind view", {**d, "m2": d["m2"][[0, 2]]}, ref)
    for v, rv in ((0, 0), (2, 1)):
        _check_cams("neighbour", d, v, ref, rv=rv)


# ---- 5. Gaussians split between two views ------------------------------------------------------------------------------------------

def _per_view_autograd(sc, cam, grads, dev):
    """the single-view GaussianRasterizer call with camera tensors that require grad: (view.grad, proj.grad, leaves' grads, m2.grad)"""
    from splatloc_amd import GaussianRasterizationSettings, GaussianRasterizer
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)  # noqa: E731
    view, proj, campos = leaf(cam.world_view_transform), leaf(cam.full_proj_transform), leaf(cam.camera_center)
    L = dict(m3=leaf(sc.means3D), col=leaf(sc.features), op=leaf(sc.opacities), sca=leaf(sc.scales), rot=leaf(sc.rotations))
    m2 = torch.zeros_like(L["m3"], requires_grad=True)
    rs = GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, sc.bg.to(dev), 1.0, view, proj, 0,
                                       campos, False, False)
    outs = GaussianRasterizer(raster_settings=rs)(means3D=L["m3"], means2D=m2, shs=None, colors_precomp=L["col"], opacities=L["op"],
                                                  scales=L["sca"], rotations=L["rot"], cov3D_precomp=None)
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs[:3], grads) if g is not None)
    loss.backward()
    torch.cuda.synchronize()
    return {"view": view.grad.cpu().numpy(), "proj": proj.grad.cpu().numpy(), "m2": m2.grad.cpu().numpy(),
            **{k: t.grad.cpu().numpy() for k, t in L.items()}}


def test_gaussians_split_between_two_views():
    """half of the Gaussians in front of view 0 only, the other half (mirrored through the origin's vertical axis) in front of
    view 2 only, which looks the other way"""
    sc = make_scene(2000, 128, 96, 4, 42, scale_median=0.04)
    flip = torch.tensor([-1.0, 1.0, -1.0])
    sc.means3D[1000:] = sc.means3D[1000:] * flip
    cams = _cameras(128, 96)[:3]
    cams[2] = PinholeCamera(128, 96, 64.0, 64.0, 63.9, 47.3, torch.diag(flip) @ _rot(0.02, -0.05), torch.tensor([0.01, 0.02, 0.1]))
    grads = _out_grads(3, 4, 96, 128, 14)
    f = _frame(sc, cams)
    radii = f.radii.cpu().numpy()
    assert (radii[0, 1000:] == 0).all() and (radii[2, :1000] == 0).all() and (radii[0, :1000] > 0).any() and (radii[2, 1000:] > 0).any()
    d = _joint(f, grads)
    one = [_per_view_autograd(sc, cams[v], grads[v], _dev()) for v in range(3)]
    for v in range(3):
        _check_cams("split", d, v, one[v], nonzero=v != 1)
    _check_params("split", d, {**{k: sum(o[k].astype(np.float64) for o in one) for k in ("m3", "col", "op", "sca", "rot")},
                               "m2": [o["m2"] for o in one]})


# ---- 6. both front ends ------------------------------------------------------------------------------------------------------------

def test_both_front_ends(scene8):
    from splatloc_amd import _native
    sc, cams, grads, ref = scene8
    got = {}
    try:
        for mode in (0, 1):
            _native.set_front_end(mode)
            got[mode] = _joint(_frame(sc, cams[:3]), grads[:3])
    finally:
        _native.set_front_end(-1)
    for mode in (0, 1):
        for v in range(3):
            _check_cams(f"front end {mode}", got[mode], v, ref[v])
        _check_params(f"front end {mode}", got[mode], _oracle_sum(ref, range(3)))


# ---- 7. V = 1 against the per-view call --------------------------------------------------------------------------------------------

def test_window_of_one_matches_splatraster_backward(scene8):
    from splatloc_amd import rasterizer as R
    sc, cams, grads, _ = scene8
    dev = _dev()
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    for v in (0, 1):        # with and without depth / alpha gradients
        d = _joint(_frame(sc, [cams[v]]), [grads[v]])
        f1 = R.view_forward(t(sc.means3D), None, t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations), None,
                            _settings(sc, [cams[v]], dev)[0])
        d1 = R.view_backward(f1, *[t(g) for g in grads[v]], want_pose=True)
        torch.cuda.synchronize()
        d1 = _np(d1)
        assert not d1["campos"].any()
        _check_cams("V=1", d, 0, d1)
        _check_params("V=1", d, {**d1, "m2": [d1["m2"]]})


# ---- 8. deterministic mode ---------------------------------------------------------------------------------------------------------

def test_deterministic_mode_gives_reproducible_parameter_gradients(scene8):
    from splatloc_amd import _native
    sc, cams, grads, ref = scene8
    _native.set_deterministic(True)
    try:
        f = _frame(sc, cams[:5])
        a, b = _joint(f, grads[:5]), _joint(f, grads[:5])
    finally:
        _native.set_deterministic(False)
    for k in ("m3", "col", "op", "sca", "rot", "m2"):
        assert np.array_equal(a[k], b[k]) and np.abs(a[k]).max() > 0, k
    print("camera gradients bit-equal between two deterministic joint backwards:",
          {k: bool(np.array_equal(a[k], b[k])) for k in ("view", "proj", "campos")})
    for v in range(5):
        _check_cams("deterministic", a, v, ref[v])
    _check_params("deterministic", a, _oracle_sum(ref, range(5)))


# ---- 9. autograd -------------------------------------------------------------------------------------------------------------------

class _Count:
    """counts the calls of one entry point of the loaded library (an instance attribute over the ctypes function)"""

    def __init__(self, lib, name):
        self.lib, self.name, self.n, self.fn = lib, name, 0, getattr(lib, name)

    def __enter__(self):
        def wrapper(*a):
            self.n += 1
            return self.fn(*a)
        setattr(self.lib, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.fn)


def _cams11(W, H):
    cams = _cameras(W, H)
    f = W / 2.0
    more = [(f, 1.02 * f, 0.03, 0.02, (0.01, 0.01, 0.08)), (0.95 * f, f, -0.01, 0.09, (-0.03, 0.02, 0.02)),
            (f, f, 0.02, -0.02, (0.04, -0.02, 0.18))]
    return cams + [PinholeCamera(W, H, fx, fy, (W - 1) / 2.0 + 0.4, (H - 1) / 2.0 - 0.2, _rot(ax, ay), torch.tensor(t))
                   for fx, fy, ax, ay, t in more]


def _window_autograd(sc, cams, grads, dev, cam_grad):
    from splatloc_amd import GaussianRasterizationSettings, rasterize_window
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)  # noqa: E731
    L = dict(m3=leaf(sc.means3D), col=leaf(sc.features), op=leaf(sc.opacities), sca=leaf(sc.scales), rot=leaf(sc.rotations))
    m2s = [torch.zeros_like(L["m3"], requires_grad=True) for _ in cams]
    bg = sc.bg.to(dev)
    ct = [tuple((leaf(x) if cam_grad else x.to(dev)) for x in (c.world_view_transform, c.full_proj_transform, c.camera_center))
          for c in cams]
    settings = [GaussianRasterizationSettings(c.image_height, c.image_width, c.tanfovx, c.tanfovy, bg, 1.0, v, p, 0, cp, False, False)
                for c, (v, p, cp) in zip(cams, ct)]
    outs = rasterize_window(settings, L["m3"], m2s, L["col"], L["op"], scales=L["sca"], rotations=L["rot"])
    loss = sum((o * g.to(dev)).sum() for out, gs in zip(outs, grads) for o, g in zip(out[:3], gs) if g is not None)
    loss.backward()
    torch.cuda.synchronize()
    return L, m2s, ct, outs


def test_rasterize_window_returns_camera_gradients_across_chunks():
    from splatloc_amd import _native
    lib = _native.load()
    dev = _dev()
    sc = make_scene(3000, 200, 120, 4, 406, scale_median=0.04)
    cams = _cams11(200, 120)
    grads = _out_grads(11, 4, 120, 200, 31, bare=(1, 9))
    with _Count(lib, "splatraster_backward_window_joint") as joint, _Count(lib, "splatraster_backward_window") as plain:
        L, m2s, ct, _ = _window_autograd(sc, cams, grads, dev, cam_grad=True)
    assert joint.n == 2 and plain.n == 0                                        # chunks of 8 + 3
    one = [_per_view_autograd(sc, cams[v], grads[v], dev) for v in range(11)]
    for v in range(11):
        d = {"view": ct[v][0].grad.cpu().numpy()[None], "proj": ct[v][1].grad.cpu().numpy()[None], "campos": ct[v][2].grad.cpu().numpy()}
        _check_cams(f"autograd view {v}", d, 0, one[v])
        assert_grad_close(f"means2D[{v}]", m2s[v].grad.cpu().numpy(), one[v]["m2"])
    for k in ("m3", "col", "op", "sca", "rot"):
        assert_grad_close(k, L[k].grad.cpu().numpy(), sum(o[k].astype(np.float64) for o in one))


def test_rasterize_window_without_camera_gradients_takes_the_plain_path():
    from splatloc_amd import _native
    lib = _native.load()
    dev = _dev()
    sc = make_scene(3000, 200, 120, 4, 406, scale_median=0.04)
    cams = _cams11(200, 120)
    grads = _out_grads(11, 4, 120, 200, 31, bare=(1, 9))
    _native.set_deterministic(True)
    try:
        with _Count(lib, "splatraster_backward_window_joint") as joint, _Count(lib, "splatraster_backward_window") as plain:
            La, m2a, cta, oa = _window_autograd(sc, cams, grads, dev, cam_grad=False)
            Lb, m2b, _, ob = _window_autograd(sc, cams, grads, dev, cam_grad=False)
    finally:
        _native.set_deterministic(False)
    assert joint.n == 0 and plain.n == 4
    assert all(t.grad is None for cam in cta for t in cam)
    for a, b in zip(oa, ob):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for k in La:
        assert torch.equal(La[k].grad, Lb[k].grad) and La[k].grad.abs().max() > 0, k
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(m2a, m2b))


# ---- 10. WindowPoses ---------------------------------------------------------------------------------------------------------------

def test_window_poses_steps_are_slot_independent_and_fixed_frames_never_move():
    from splatloc_amd import pose
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    N = 11
    W2C0 = pose.at_to_transform_matrix(0.3 * torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)).contiguous().to(dev)
    Pm = torch.randn(4, 4, generator=g).to(dev)
    G = [(torch.randn(N, 4, 4, generator=g).to(dev), torch.randn(N, 4, 4, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev))
         for _ in range(3)]
    orders = [list(range(N)), [7, 2, 10, 0, 5, 3, 9, 1, 8, 6, 4]]          # neighbouring rows in place / gathered slots, 8 + 3

    def run(order, fixed=()):
        wp = pose.WindowPoses(W2C0, Pm, lr_rot=2e-2, lr_trans=3e-2, fixed=fixed)
        start = [t.detach().clone() for t in (wp.view, wp.proj, wp.campos)]
        for gv, gp, gc in G:
            wp.view.grad, wp.proj.grad, wp.campos.grad = gv.clone(), gp.clone(), gc.clone()
            wp.step(order)
            assert not wp.view.grad.any() and not wp.proj.grad.any() and not wp.campos.grad.any()
        torch.cuda.synchronize()
        return wp, start

    (a, start), (b, _) = run(orders[0]), run(orders[1])
    assert a.view.requires_grad and a.view.is_leaf and a.proj.is_leaf and a.campos.is_leaf
    for x, y in ((a.state, b.state), (a.view, b.view), (a.proj, b.proj), (a.campos, b.campos)):
        for j in range(N):
            assert torch.equal(x[j], y[j]), j
    assert (a.state[:, 18] == 3).all() and (a.view.detach() - start[0]).abs().amax(dim=(1, 2)).min() > 0
    # the start tensors are those of W2C_init, and W2C() those of the state
    for j in (0, N - 1):
        vr, pr, cr = pose.camera_tensors(W2C0[j].double(), Pm.double())
        assert torch.allclose(start[0][j].double(), vr, atol=2e-6) and torch.allclose(start[1][j].double(), pr, atol=1e-5)
        assert torch.allclose(start[2][j].double(), cr, atol=1e-5)
        assert torch.allclose(a.W2C()[j].T, a.view[j].detach(), atol=2e-5)
    v5, p5, c5 = a.cameras(5)
    assert v5.data_ptr() == a.view[5].data_ptr() and p5.shape == (4, 4) and c5.shape == (3,) and len(a.cameras([1, 2])) == 2
    # fixed frames: never moved, whatever the order; the others as without `fixed`
    (c, start_c), _ = run(orders[1], fixed=[2, 9]), None
    for j in range(N):
        if j in (2, 9):
            assert not c.state[j].any() and torch.equal(c.view[j], start_c[0][j]) and torch.equal(c.proj[j], start_c[1][j])
            assert torch.equal(c.W2C()[j], W2C0[j])
        else:
            assert torch.equal(c.state[j], a.state[j]) and torch.equal(c.view[j], a.view[j])
    with pytest.raises(ValueError, match="distinct"):
        a.step([1, 1])


# ---- 11. end to end: key-frame poses optimised together with the map ---------------------------------------------------------------

def _targets(sc, cam, W2C_true):
    from splatloc_amd import GaussianRasterizationSettings, GaussianRasterizer, pose
    cs, ds = [], []
    with torch.no_grad():
        for M in W2C_true:
            view, proj, campos = pose.camera_tensors(M, cam.projection_matrix)
            rs = GaussianRasterizationSettings(192, 256, cam.tanfovx, cam.tanfovy, sc.bg, 1.0, view, proj, 0, campos, False, False)
            c, d, _, _ = GaussianRasterizer(raster_settings=rs)(
                means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), shs=None, colors_precomp=sc.features,
                opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations, cov3D_precomp=None)
            cs.append(c)
            ds.append(d)
    return torch.stack(cs), torch.stack(ds)


def test_key_frame_poses_and_map_are_optimised_together():
    """test_refine_poses_recovers_three_perturbed_cameras' scene, perturbations, learning rates, iteration count and criteria; here
    the three frames are key-frames of a window of five (two more frames at their true poses, `fixed`: the gauge), and the map's
    colours and opacities start slightly wrong and train with Adam in the same iterations (positions held)."""
    from splatloc_amd import GaussianRasterizationSettings, _native, pose, rasterize_window
    lib = _native.load()
    dev = _dev()
    sc = make_scene(6000, 256, 192, 3, 81, scale_median=0.05).to(dev)
    cam = PinholeCamera(256, 192, 128.0, 128.0, 127.5, 95.5)
    cam.to(dev)
    w_true = torch.tensor([[0.02, -0.03, 0.01], [-0.015, 0.02, 0.02], [0.01, 0.025, -0.02], [0.03, 0.01, 0.0], [-0.02, -0.01, 0.01]],
                          device=dev)
    t_true = torch.tensor([[0.03, -0.02, 0.05], [-0.03, 0.03, 0.04], [0.02, 0.04, -0.03], [0.05, 0.0, 0.02], [-0.04, 0.02, 0.0]],
                          device=dev)
    W2C_true = pose.at_to_transform_matrix(w_true, t_true)
    tgt_c, tgt_d = _targets(sc, cam, W2C_true)
    eye = torch.eye(4, device=dev)
    W2C0 = torch.stack([eye, eye, eye, W2C_true[3], W2C_true[4]])
    poses = pose.WindowPoses(W2C0, cam.projection_matrix, fixed=[3, 4])        # refine_poses' learning rates and betas
    gen = torch.Generator().manual_seed(3)
    colors = (sc.features + 0.03 * torch.randn(sc.features.shape, generator=gen).to(dev)).clamp(0.0, 1.0).requires_grad_(True)
    op_logit = (torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)) + 0.2 * torch.randn(sc.opacities.shape, generator=gen).to(dev)).requires_grad_(True)
    opt = torch.optim.Adam([colors, op_logit], lr=2e-3)
    settings = [GaussianRasterizationSettings(192, 256, cam.tanfovx, cam.tanfovy, sc.bg, 1.0, v, p, 0, c, False, False)
                for v, p, c in poses.cameras(range(5))]
    m2 = [torch.zeros_like(sc.means3D) for _ in range(5)]
    iterations = 150
    hist = torch.zeros((iterations, 5), device=dev)
    col_hist = torch.zeros((iterations,), device=dev)
    with _Count(lib, "splatraster_backward_window_joint") as joint, _Count(lib, "splatraster_forward_window_render") as fwd, \
            _Count(lib, "splatraster_backward_window") as plain, _Count(lib, "splatraster_backward_window_cameras") as camsonly, \
            _Count(lib, "splatraster_backward") as single:
        for it in range(iterations):
            outs = rasterize_window(settings, sc.means3D, m2, colors, torch.sigmoid(op_logit), scales=sc.scales, rotations=sc.rotations)
            lc = torch.stack([(o[0] - tgt_c[j]).abs().mean() for j, o in enumerate(outs)])
            ld = torch.stack([(o[1] - tgt_d[j]).abs().mean() for j, o in enumerate(outs)])
            per_frame = lc + 0.2 * ld
            opt.zero_grad(set_to_none=True)
            per_frame.sum().backward()
            opt.step()
            poses.step(range(5))
            hist[it], col_hist[it] = per_frame.detach(), lc.detach().sum()
    torch.cuda.synchronize()
    assert joint.n == iterations and fwd.n == iterations and plain.n == 0 and camsonly.n == 0 and single.n == 0
    hist, col_hist, W2C = hist.cpu(), col_hist.cpu(), poses.W2C()
    assert torch.isfinite(hist).all()

    def err(M, T):
        dR = M[:3, :3] @ T[:3, :3].T
        ang = torch.acos(((torch.trace(dR) - 1) / 2).clamp(-1, 1))
        return float(ang) + float((M[:3, 3] - T[:3, 3]).norm())
    for j in range(3):
        e0, e1 = err(eye, W2C_true[j]), err(W2C[j], W2C_true[j])
        print(f"frame {j}: loss {float(hist[0, j]):.5f} -> {float(hist[-1, j]):.5f}, pose error {e0:.4f} -> {e1:.4f}")
        assert float(hist[-1, j]) < 0.35 * float(hist[0, j]), (j, float(hist[0, j]), float(hist[-1, j]))
        assert e1 < 0.35 * e0, (j, e0, e1)
    for j in (3, 4):
        assert torch.equal(W2C[j], W2C_true[j])                                 # fixed: never moved
    print(f"colour loss {float(col_hist[0]):.5f} -> {float(col_hist[-1]):.5f}")
    assert float(col_hist[-1]) < float(col_hist[0])
