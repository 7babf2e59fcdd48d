"""Pose refinement of a window of query frames on the GPU: the camera gradients of every view of a window
(splatraster_backward_window_cameras, csrc/camera_bwd.hip) against the oracle and against the per-view call, at the kernel's
block / set / view edges; the loss and the Adam step of a window (csrc/pose.hip) against their single-frame forms; and
pose.refine_poses end to end and against pose.refine_pose frame by frame."""
import ctypes as C
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
    gc, gd, ga = grads
    s = dataclasses.replace(sc, camera=cam, dL_dcolor=gc, dL_ddepth=gd, dL_dalpha=ga)
    f = oracle_forward(s)
    b = oracle_backward(f, s, use_depth=gd is not None, use_alpha=ga is not None)
    return {"view": b["dL_dviewmatrix"], "proj": b["dL_dprojmatrix"], "R": int(f["num_rendered"])}


def _settings(sc, cams, dev):
    from splatloc_amd import GaussianRasterizationSettings
    bg = sc.bg.to(dev)
    return [GaussianRasterizationSettings(c.image_height, c.image_width, c.tanfovx, c.tanfovy, bg, 1.0,
                                          c.world_view_transform.to(dev), c.full_proj_transform.to(dev), 0, c.camera_center.to(dev),
                                          False, False) for c in cams]


def _window(sc, cams, grads, dev=None):
    """window_forward + window_backward_cameras of `cams` over the scene: (frame, {view, proj, campos} as numpy)"""
    from splatloc_amd import rasterizer as R
    dev = dev or torch.device("cuda:0")
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    f = R.window_forward(t(sc.means3D), t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations), None,
                         _settings(sc, cams, dev))
    d = R.window_backward_cameras(f, [tuple(t(g) for g in gs) for gs in grads])
    torch.cuda.synchronize()
    assert set(d) == {"view", "proj", "campos"}
    assert d["view"].shape == (len(cams), 4, 4) and d["proj"].shape == (len(cams), 4, 4) and d["campos"].shape == (len(cams), 3)
    return f, {k: v.cpu().numpy() for k, v in d.items()}


def _check(name, d, v, ref, nonzero=True):
    if nonzero:
        assert float(np.abs(ref["view"]).max()) > 0 and float(np.abs(ref["proj"]).max()) > 0     # cannot pass on zeros
    assert_grad_close(f"{name} dL_dviewmatrix[{v}]", d["view"][v], ref["view"], **TOL)
    assert_grad_close(f"{name} dL_dprojmatrix[{v}]", d["proj"][v], ref["proj"], **TOL)
    assert not d["campos"].any()


@pytest.fixture(scope="module")
def scene8():
    """the scene of test_pose_gradients_match_oracle, eight cameras, their output gradients and the oracle's answer per view"""
    sc = make_scene(3000, 256, 192, 4, 70, scale_median=0.03)
    cams = _cameras(256, 192)
    grads = _out_grads(8, 4, 192, 256, 11)
    return sc, cams, grads, [_oracle(sc, c, g) for c, g in zip(cams, grads)]


@pytest.mark.parametrize("V", [1, 2, 3, 8])
def test_window_camera_gradients_match_the_oracle_per_view(scene8, V):
    sc, cams, grads, ref = scene8
    assert len({(c.tanfovx, c.tanfovy) for c in cams[:2]}) == 2
    f, d = _window(sc, cams[:V], grads[:V])
    assert f.R == [r["R"] for r in ref[:V]]
    for v in range(V):
        _check(f"V={V}", d, v, ref[v])


def test_window_camera_gradients_match_the_per_view_call(scene8):
    """both are f32 sums of the same partials in different orders: the per-view call is the reference here"""
    from splatloc_amd import rasterizer as R
    sc, cams, grads, _ = scene8
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    _, d = _window(sc, cams, grads)
    for v, rs in enumerate(_settings(sc, cams, dev)):
        f1 = R.view_forward(t(sc.means3D), None, t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations), None, rs)
        d1 = R.view_backward(f1, *[t(g) for g in grads[v]], want_pose=True)
        torch.cuda.synchronize()
        one = {"view": d1["view"].cpu().numpy(), "proj": d1["proj"].cpu().numpy()}
        _check("vs V=1", d, v, one)
        assert not d1["campos"].cpu().numpy().any()


@pytest.mark.parametrize("P", [1, 255, 256, 257, 4353, 0])
def test_block_and_set_edges(P):
    """one thread, one short of / exactly / one past a block, and 18 blocks per view: more than the 16 sets, two of which then
    take two blocks (uneven tickets); no Gaussians at all"""
    sc = make_scene(P, 64, 48, 4, 300 + P % 7, scale_median=0.05)
    if P == 1:      # the one Gaussian in front of all three cameras
        sc.means3D = torch.tensor([[0.1, -0.05, 2.0]])
    cams = _cameras(64, 48)[:3]
    grads = _out_grads(3, 4, 48, 64, 12)
    f, d = _window(sc, cams, grads)
    if P == 0:
        assert f.R == [0, 0, 0] and not d["view"].any() and not d["proj"].any() and not d["campos"].any()
        return
    for v in range(3):
        ref = _oracle(sc, cams[v], grads[v])
        assert f.R[v] == ref["R"] and ref["R"] > 0
        _check(f"P={P}", d, v, ref)


def test_a_view_that_sees_nothing_writes_zeros():
    sc = make_scene(2000, 128, 96, 4, 41, scale_median=0.04)
    cams = _cameras(128, 96)[:3]
    f = 64.0
    cams[1] = PinholeCamera(128, 96, f, f, 63.9, 47.3, torch.diag(torch.tensor([-1.0, 1.0, -1.0])), torch.tensor([0.02, 0.0, 0.1]))
    grads = _out_grads(3, 4, 96, 128, 13, bare=())
    fr, d = _window(sc, cams, grads)
    assert fr.R[1] == 0 and fr.R[0] > 0 and fr.R[2] > 0
    assert not d["view"][1].any() and not d["proj"][1].any() and not d["campos"][1].any()       # all 35, exactly
    for v in (0, 2):
        _check("neighbour", d, v, _oracle(sc, cams[v], grads[v]))


def test_gaussians_split_between_two_views():
    """half of the Gaussians in front of view 0 only, the other half (mirrored through the origin's vertical axis) in front of
    view 2 only, which looks the other way"""
    sc = make_scene(2000, 128, 96, 4, 42, scale_median=0.04)
    flip = torch.tensor([-1.0, 1.0, -1.0])
    sc.means3D[1000:] = sc.means3D[1000:] * flip
    cams = _cameras(128, 96)[:3]
    cams[2] = PinholeCamera(128, 96, 64.0, 64.0, 63.9, 47.3, torch.diag(flip) @ _rot(0.02, -0.05), torch.tensor([0.01, 0.02, 0.1]))
    grads = _out_grads(3, 4, 96, 128, 14)
    fr, d = _window(sc, cams, grads)
    radii = fr.radii.cpu().numpy()
    assert (radii[0, 1000:] == 0).all() and (radii[2, :1000] == 0).all() and (radii[0, :1000] > 0).any() and (radii[2, 1000:] > 0).any()
    for v in range(3):
        _check("split", d, v, _oracle(sc, cams[v], grads[v]), nonzero=v != 1)


def test_a_cameras_result_does_not_depend_on_its_slot():
    """deterministic accumulator rows, one block per view (a fixed summation order): the 35 outputs of a camera are the same
    bits at slot 2 of one window and at slot 6 of another"""
    from splatloc_amd import _native
    sc = make_scene(200, 64, 48, 4, 43, scale_median=0.05)
    cams = _cameras(64, 48)
    grads = _out_grads(8, 4, 48, 64, 15)
    order_a, order_b = [0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 1, 2, 0]       # camera 2: slot 2, then slot 6
    _native.set_deterministic(True)
    try:
        _, da = _window(sc, [cams[i] for i in order_a], [grads[i] for i in order_a])
        _, db = _window(sc, [cams[i] for i in order_b], [grads[i] for i in order_b])
    finally:
        _native.set_deterministic(False)
    assert order_a[2] == order_b[6] == 2 and np.abs(da["view"][2]).max() > 0
    for k in ("view", "proj", "campos"):
        assert np.array_equal(da[k][2], db[k][6]), k


def test_both_front_ends(scene8):
    from splatloc_amd import _native
    sc, cams, grads, ref = scene8
    got = {}
    try:
        for mode in (0, 1):
            _native.set_front_end(mode)
            _, got[mode] = _window(sc, cams[:3], grads[:3])
    finally:
        _native.set_front_end(-1)
    for v in range(3):
        for mode in (0, 1):
            _check(f"front end {mode}", got[mode], v, ref[v])
        _check("binned vs radix", got[1], v, {k: got[0][k][v] for k in ("view", "proj")})


# ---- the loss of a window ------------------------------------------------------------------------------------------------

def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("V", [1, 3, 8])
def test_l1_rgbd_loss_window_matches_single_calls(V, odd):
    from splatloc_amd import _native
    lib = _native.load()
    dev = torch.device("cuda:0")
    n_c, n_d = (3 * 61 * 47, 61 * 47) if odd else (4 * 64 * 48, 64 * 48)   # odd: the views' planes are not 16-byte aligned
    g = torch.Generator().manual_seed(20 + V)
    col, tc = torch.rand(V, n_c, generator=g).to(dev), torch.rand(V, n_c, generator=g).to(dev)
    dep, td = torch.rand(V, n_d, generator=g).to(dev), torch.rand(V, n_d, generator=g).to(dev)
    tc[:, ::7] = col[:, ::7]        # exact zeros of the difference: gradient 0
    assert (not odd) or any(col[v].data_ptr() % 16 for v in range(V)) or V == 1
    for with_depth in (True, False):
        gc1, gd1, l1 = torch.empty(V, n_c, device=dev), torch.ones(V, n_d, device=dev), torch.zeros(V, device=dev)
        for v in range(V):
            _native.check(lib.splatraster_l1_rgbd_loss(n_c, _ptr(col[v]), _ptr(tc[v]), n_d, _ptr(dep[v]),
                                                       _ptr(td[v]) if with_depth else None, 0.2, _ptr(gc1[v]), _ptr(gd1[v]),
                                                       C.c_void_p(l1.data_ptr() + 4 * v), None), "l1")
        gcw, gdw, lw = torch.empty(V, n_c, device=dev), torch.ones(V, n_d, device=dev), torch.zeros(V, device=dev)
        lv = (_native.L1View * V)()
        for v in range(V):
            lv[v].color, lv[v].target_color, lv[v].depth = col[v].data_ptr(), tc[v].data_ptr(), dep[v].data_ptr()
            lv[v].target_depth = td[v].data_ptr() if with_depth else None
            lv[v].g_color, lv[v].g_depth = gcw[v].data_ptr(), gdw[v].data_ptr()
        _native.check(lib.splatraster_l1_rgbd_loss_window(V, lv, n_c, n_d, 0.2, _ptr(lw), None), "l1_window")
        torch.cuda.synchronize()
        assert torch.equal(gcw, gc1) and torch.equal(gdw, gd1)
        assert (gcw[:, ::7] == 0).all() and gcw.abs().max() > 0
        if not with_depth:
            assert not gdw.any()                                             # no depth target: the plane is zeroed
        l1, lw = l1.cpu().double(), lw.cpu().double()
        print(f"V={V} odd={odd} depth={with_depth}: max rel |window - single| = {float(((lw - l1).abs() / l1).max()):.2e}")
        assert (l1 > 0).all() and ((lw - l1).abs() <= 2e-6 * l1).all()


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
def test_the_single_view_l1_entry_is_the_window_kernel(offset, with_depth):
    """splatraster_l1_rgbd_loss launches l1_rgbd_loss_window_kernel with one view.  Colour 3x5x7 = 105 elements (26 float4 and a
    tail of one) and depth 1x5x7 are ONE block, so the loss is summed in one fixed order and can be compared bit for bit:
    the single-view call, the window call at V = 1 and view 3 of a window of eight whose other views hold other data give the
    same loss word and the same gradient planes.  offset = 1: colour, target and gradient start one float behind a 16-byte
    boundary, which takes the kernel's scalar path.  The loss itself: within 2e-6 of a float64 sum, the bound of
    test_l1_rgbd_loss_window_matches_single_calls (at most 12 float32 roundings per partial sum here: 7e-7)."""
    from splatloc_amd import _native
    lib = _native.load()
    dev = torch.device("cuda:0")
    n_c, n_d, V, slot, wd = 3 * 5 * 7, 5 * 7, 8, 3, 0.2
    g = torch.Generator().manual_seed(41 + offset)
    pad = 4 + ((n_c + 3) & ~3)                     # a view's row: 16-byte aligned, room for the offset
    col, tc = torch.rand(V, pad, generator=g).to(dev), torch.rand(V, pad, generator=g).to(dev)
    dep, td = torch.rand(V, 36, generator=g).to(dev), torch.rand(V, 36, generator=g).to(dev)
    tc[:, offset:offset + n_c:7] = col[:, offset:offset + n_c:7]      # exact zeros of the difference: gradient 0
    assert all(t[v].data_ptr() % 16 == 0 for t in (col, tc, dep, td) for v in range(V))

    def view(lv, k, v, gc, gd):
        lv[k].color, lv[k].target_color = col[v].data_ptr() + 4 * offset, tc[v].data_ptr() + 4 * offset
        lv[k].depth, lv[k].target_depth = dep[v].data_ptr(), td[v].data_ptr() if with_depth else None
        lv[k].g_color, lv[k].g_depth = gc.data_ptr() + 4 * offset, gd.data_ptr()

    def planes(n):
        return torch.full((n, pad), 7.0, device=dev), torch.ones(n, 36, device=dev), torch.zeros(n, device=dev)

    gc1, gd1, l1 = planes(1)
    _native.check(lib.splatraster_l1_rgbd_loss(n_c, C.c_void_p(col[slot].data_ptr() + 4 * offset), C.c_void_p(tc[slot].data_ptr() + 4 * offset),
                                               n_d, _ptr(dep[slot]), _ptr(td[slot]) if with_depth else None, wd,
                                               C.c_void_p(gc1.data_ptr() + 4 * offset), _ptr(gd1), _ptr(l1), None), "l1")
    gcw, gdw, lw = planes(1)
    lv = (_native.L1View * 1)()
    view(lv, 0, slot, gcw[0], gdw[0])
    _native.check(lib.splatraster_l1_rgbd_loss_window(1, lv, n_c, n_d, wd, _ptr(lw), None), "l1_window 1")
    gc8, gd8, l8 = planes(V)
    lv = (_native.L1View * V)()
    for v in range(V):
        view(lv, v, v, gc8[v], gd8[v])
    _native.check(lib.splatraster_l1_rgbd_loss_window(V, lv, n_c, n_d, wd, _ptr(l8), None), "l1_window 8")
    torch.cuda.synchronize()
    for name, gc, gd, loss in (("V = 1", gcw[0], gdw[0], lw), ("view 3 of 8", gc8[slot], gd8[slot], l8[slot:slot + 1])):
        assert torch.equal(gc, gc1[0]) and torch.equal(gd, gd1[0]), name
        assert torch.equal(loss.view(torch.int32), l1.view(torch.int32)), (name, float(loss), float(l1))
    assert not torch.equal(gc8[0], gc8[slot]) and l8[0] != l8[slot]            # the other views did hold other data
    own = gc1[0, offset:offset + n_c]
    assert (own[::7] == 0).all() and own.abs().max() > 0 and (gc1[0, :offset] == 7).all() and (gc1[0, offset + n_c:] == 7).all()
    assert (gd1[0, n_d:] == 1).all()                                            # nothing written behind the planes
    if not with_depth:
        assert not gd1[0, :n_d].any()                                           # no depth target: the plane is zeroed
    x, t = col[slot, offset:offset + n_c].cpu().double().numpy(), tc[slot, offset:offset + n_c].cpu().double().numpy()
    ref = np.abs(x - t).sum() / n_c
    if with_depth:
        ref += wd * np.abs(dep[slot, :n_d].cpu().double().numpy() - td[slot, :n_d].cpu().double().numpy()).sum() / n_d
    print(f"offset={offset} depth={with_depth}: loss {float(l1[0]):.9g}, float64 {ref:.9g}, rel {abs(float(l1[0]) - ref) / ref:.2e}")
    assert abs(float(l1[0]) - ref) <= 2e-6 * ref


# ---- the Adam step of a window ---------------------------------------------------------------------------------------------

def test_pose_step_window_matches_autograd_adam_and_is_slot_independent():
    """the protocol of test_pose_step_kernel_matches_autograd_and_torch_adam for eight cameras with different start poses: random
    upstream gradients, three steps, float64 autograd + torch.optim.Adam per camera; the same cameras again in other slots of
    smaller windows: the same bits; and through the single-camera kernel"""
    from splatloc_amd import _native, pose
    lib = _native.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    W2C0 = pose.at_to_transform_matrix(0.3 * torch.randn(8, 3, generator=g), torch.randn(8, 3, generator=g)).contiguous()
    Pm = torch.randn(4, 4, generator=g)
    G = [(torch.randn(8, 4, 4, generator=g), torch.randn(8, 4, 4, generator=g), torch.randn(8, 3, generator=g)) for _ in range(3)]
    lr = (2e-2, 3e-2)

    def run(ids):
        """the cameras `ids` as one window: [(view, proj, campos, state) after step(0) and after each of the three steps]"""
        n, sel = len(ids), torch.tensor(ids)
        w0, pm = W2C0[sel].contiguous().to(dev), Pm.to(dev)
        state = torch.zeros(n, 20, device=dev)
        view, proj, campos = torch.empty(n, 4, 4, device=dev), torch.empty(n, 4, 4, device=dev), torch.empty(n, 3, device=dev)
        snaps = []

        def step(adv, gs=(None, None, None)):
            gs = [None if x is None else x[sel].contiguous().to(dev) for x in gs]
            _native.check(lib.splatraster_pose_step_window(n, _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(w0), _ptr(pm), lr[0], lr[1],
                                                           0.9, 0.999, 1e-8, adv, _ptr(state), _ptr(view), _ptr(proj), _ptr(campos),
                                                           None), "pose_step_window")
            torch.cuda.synchronize()
            snaps.append(tuple(x.cpu().clone() for x in (view, proj, campos, state)))
        step(0)
        for gs in G:
            step(1, gs)
        return snaps

    full = run(list(range(8)))
    # advance = 0: the tensors of the initial state, the state itself untouched
    v0, p0, c0, s0 = full[0]
    assert not s0.any()
    for c in range(8):
        vr, pr, cr = pose.camera_tensors(W2C0[c].double(), Pm.double())
        assert torch.allclose(v0[c].double(), vr, atol=2e-6) and torch.allclose(p0[c].double(), pr, atol=1e-5)
        assert torch.allclose(c0[c].double(), cr, atol=1e-5)
    # float64 autograd + torch.optim.Adam, camera by camera
    for c in range(8):
        w = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
        t = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([{"params": [w], "lr": lr[0]}, {"params": [t], "lr": lr[1]}])
        for k, (Gv, Gp, Gc) in enumerate(G):
            vr, pr, cr = pose.camera_tensors(pose.at_to_transform_matrix(w, t)[0] @ W2C0[c].double(), Pm.double())
            view, proj, campos, _ = full[k]
            assert torch.allclose(view[c].double(), vr.detach(), atol=2e-6) and torch.allclose(proj[c].double(), pr.detach(), atol=1e-5)
            assert torch.allclose(campos[c].double(), cr.detach(), atol=1e-5)
            loss = (vr * Gv[c].double()).sum() + (pr * Gp[c].double()).sum() + (cr * Gc[c].double()).sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
            st = full[k + 1][3][c].double()
            assert torch.allclose(st[:3], w.detach()[0], atol=2e-6), (c, k, st[:3], w)
            assert torch.allclose(st[3:6], t.detach()[0], atol=2e-6), (c, k, st[3:6], t)
            assert float(st[18]) == k + 1
    # whichever slot, whichever n
    for ids in ([5, 0, 7], [2, 7, 5], [5]):
        part = run(ids)
        for k in range(4):
            for slot, c in enumerate(ids):
                for a, b in zip(part[k], full[k]):
                    assert torch.equal(a[slot], b[c]), (ids, k, slot)
    # and the single-camera kernel: the same statements in another instantiation (the compiler may contract them differently, so
    # this comparison has that test's bounds; whether the bits agree is printed)
    c = 5
    w0, pm, state = W2C0[c].contiguous().to(dev), Pm.to(dev), torch.zeros(20, device=dev)
    view, proj, campos = torch.empty(4, 4, device=dev), torch.empty(4, 4, device=dev), torch.empty(3, device=dev)
    for k in range(4):
        gs = [None] * 3 if k == 0 else [x[c].contiguous().to(dev) for x in G[k - 1]]
        _native.check(lib.splatraster_pose_step(_ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(w0), _ptr(pm), lr[0], lr[1], 0.9, 0.999, 1e-8,
                                                int(k > 0), _ptr(state), _ptr(view), _ptr(proj), _ptr(campos), None), "pose_step")
        torch.cuda.synchronize()
        for a, b, tol in zip((view, proj, campos, state), full[k], (2e-6, 1e-5, 1e-5, 2e-6)):
            print(f"single vs window, step {k}: bit-identical = {torch.equal(a.cpu(), b[c])}")
            assert torch.allclose(a.cpu(), b[c], rtol=0.0, atol=tol), k


# ---- refine_poses ------------------------------------------------------------------------------------------------------------

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


def test_refine_poses_recovers_three_perturbed_cameras():
    """test_refine_pose_recovers_a_perturbed_camera's scene and criteria, per frame, for three frames with different true poses
    refined as one window"""
    from splatloc_amd import pose
    dev = torch.device("cuda:0")
    sc = make_scene(6000, 256, 192, 3, 81, scale_median=0.05).to(dev)
    cam = PinholeCamera(256, 192, 128.0, 128.0, 127.5, 95.5)
    cam.to(dev)
    w_true = torch.tensor([[0.02, -0.03, 0.01], [-0.015, 0.02, 0.02], [0.01, 0.025, -0.02]], device=dev)
    t_true = torch.tensor([[0.03, -0.02, 0.05], [-0.03, 0.03, 0.04], [0.02, 0.04, -0.03]], device=dev)
    W2C_true = pose.at_to_transform_matrix(w_true, t_true)
    tgt = _targets(sc, cam, W2C_true)
    g = dict(means3D=sc.means3D, colors=sc.features, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations)
    eye = torch.eye(4, device=dev)
    W2C, hist = pose.refine_poses(tgt, g, cam, eye.repeat(3, 1, 1), iterations=150, background=sc.bg, window=8)
    hist = hist.cpu()
    assert W2C.shape == (3, 4, 4) and hist.shape == (150, 3) and torch.isfinite(hist).all()

    def err(M, T):
        dR = M[:3, :3] @ T[:3, :3].T
        ang = torch.acos(((torch.trace(dR) - 1) / 2).clamp(-1, 1))
        return float(ang) + float((M[:3, 3] - T[:3, 3]).norm())
    for j in range(3):
        e0, e1 = err(eye, W2C_true[j]), err(W2C[j], W2C_true[j])
        print(f"frame {j}: loss {float(hist[0, j]):.5f} -> {float(hist[-1, j]):.5f}, pose error {e0:.4f} -> {e1:.4f}")
        assert float(hist[-1, j]) < 0.35 * float(hist[0, j]), (j, float(hist[0, j]), float(hist[-1, j]))
        assert e1 < 0.35 * e0, (j, e0, e1)


def test_refine_poses_follows_refine_pose_frame_by_frame():
    """eleven frames, window 8 (chunks of 8 and 3), 40 iterations: every frame against refine_pose of that frame alone — same
    start, same settings — within test_graph_free_refine_pose_follows_the_autograd_loop's bounds"""
    from splatloc_amd import pose
    dev = torch.device("cuda:0")
    sc = make_scene(6000, 256, 192, 3, 81, scale_median=0.05).to(dev)
    cam = PinholeCamera(256, 192, 128.0, 128.0, 127.5 + 0.3, 95.5 - 0.2)
    cam.to(dev)
    gen = torch.Generator().manual_seed(9)
    N = 11
    W2C_true = pose.at_to_transform_matrix(0.02 * torch.randn(N, 3, generator=gen), 0.04 * torch.randn(N, 3, generator=gen)).to(dev)
    W2C0 = pose.at_to_transform_matrix(0.015 * torch.randn(N, 3, generator=gen), 0.02 * torch.randn(N, 3, generator=gen)).to(dev)
    tgt_c, tgt_d = _targets(sc, cam, W2C_true)
    g = dict(means3D=sc.means3D, colors=sc.features, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations)
    Ww, hw = pose.refine_poses((tgt_c, tgt_d), g, cam, W2C0, iterations=40, background=sc.bg, window=8)
    hw = hw.cpu().double()
    assert Ww.shape == (N, 4, 4) and hw.shape == (40, N) and torch.isfinite(hw).all()
    for j in range(N):
        W1, h1 = pose.refine_pose((tgt_c[j], tgt_d[j]), g, cam, W2C0[j], iterations=40, background=sc.bg)
        h1 = h1.cpu().double()
        dl0, dh = abs(float(h1[0] - hw[0, j])) / float(h1[0]), float((h1 - hw[:, j]).abs().max()) / float(h1[0])
        dW = float((W1 - Ww[j]).abs().max())
        print(f"frame {j}: first loss rel {dl0:.2e}, history {dh:.2e} of the first loss, pose {dW:.2e}")
        assert dl0 <= 2e-6 and dh <= 2e-3 and dW <= 2e-4, (j, dl0, dh, dW)
