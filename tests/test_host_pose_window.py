"""Host-side checks of the pose refinement of a window of frames (csrc/camera_bwd.hip, csrc/pose.hip, pose.refine_poses): the new
entry points are declared and bound, the workspace size, every argument error of the three entry points is returned before any
device work, refine_poses' ValueErrors, and the chunking arithmetic."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from splatloc_amd import _native, pose

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "splatraster.h")
NEW = ("splatraster_window_camera_workspace_bytes", "splatraster_backward_window_cameras", "splatraster_l1_rgbd_loss_window",
       "splatraster_pose_step_window")


def test_new_symbols_are_declared_and_bound():
    text = open(HEADER).read()
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", text), name
        assert name in _native.SYMBOLS and getattr(lib, name).argtypes == _native.SYMBOLS[name][1]
    assert "typedef struct splatraster_l1_view" in text
    assert [n for n, _ in _native.L1View._fields_] == ["color", "target_color", "depth", "target_depth", "g_color", "g_depth"]
    assert _native.ABI_VERSION == 20 and lib.splatraster_abi_version() == 20        # new symbols only


def test_camera_workspace_bytes():
    ws = _native.load().splatraster_window_camera_workspace_bytes
    sizes = [ws(v) for v in range(1, 9)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    # per view: sixteen sets of 27 partial sums, each with its ticket, and the view's ticket
    assert sizes[0] >= 16 * 28 * 4 + 4 and sizes[7] == 8 * sizes[0]
    for v in (0, -1, 9, 1 << 20):
        assert ws(v) == 0


def _host_ptr():
    """host memory: a launch or a memset on it would fault, an argument check returns first"""
    cell = (C.c_float * 64)(*([7.0] * 64))
    return cell, C.cast(cell, C.c_void_p)


def test_backward_window_cameras_bad_arguments_return_before_any_launch():
    lib = _native.load()
    cell, p = _host_ptr()
    st = _native.Settings(48, 64, 1.0, 1.0, 1.0, 0, 0, 4, 0, 0, 0)
    views = (_native.WindowView * 8)()
    for w in views:
        w.viewmatrix = w.projmatrix = w.radii = w.out_color = w.out_depth = w.out_alpha = w.dL_dout_color = p.value
        w.tanfovx = w.tanfovy = 1.0
    R = (C.c_int64 * 8)(*([5] * 8))
    call = lib.splatraster_backward_window_cameras

    def args(s=C.byref(st), V=2, vw=views, P=10, R_=R, ws=p, dv=p, dp=p, m3=p, col=p, sca=p, rot=p, cov=None, geom=p, binning=p, img=p):
        return (s, V, vw, P, R_, None, m3, col, sca, rot, cov, geom, binning, img, ws, dv, dp, None, None)
    for V in (0, -3, 9):
        assert call(*args(V=V)) == 1
    assert call(*args(s=None)) == 1 and call(*args(vw=None)) == 1 and call(*args(R_=None)) == 1
    assert call(*args(ws=None)) == 1 and call(*args(dv=None)) == 1 and call(*args(dp=None)) == 1
    assert call(*args(P=-1)) == 1
    assert call(*args(ws=None, P=0)) == 1 and call(*args(dv=None, P=0)) == 1      # also when there is nothing to differentiate
    for k in ("m3", "col", "geom", "binning", "img", "sca", "rot"):
        assert call(*args(**{k: None})) == 1, k
    assert call(*args(cov=p)) == 1                                              # scales + rotations AND a covariance
    Rn = (C.c_int64 * 8)(5, -1, 5, 5, 5, 5, 5, 5)
    assert call(*args(R_=Rn)) == 1
    for field in ("viewmatrix", "projmatrix", "radii", "out_color", "out_depth", "dL_dout_color"):
        keep = getattr(views[1], field)
        setattr(views[1], field, None)
        assert call(*args()) == 1, field
        setattr(views[1], field, keep)
    views[1].color_grad_channels = 9                                            # more gradient planes than channels
    assert call(*args()) == 1
    views[1].color_grad_channels = 0
    assert all(x == 7.0 for x in cell)


def test_loss_and_step_window_bad_arguments_return_before_any_launch():
    lib = _native.load()
    cell, p = _host_ptr()
    lv = (_native.L1View * 8)()
    for w in lv:
        w.color = w.target_color = w.depth = w.target_depth = w.g_color = w.g_depth = p.value
    loss = lib.splatraster_l1_rgbd_loss_window
    for V in (0, -1, 9):
        assert loss(V, lv, 16, 4, 0.2, p, None) == 1
    assert loss(2, None, 16, 4, 0.2, p, None) == 1 and loss(2, lv, 16, 4, 0.2, None, None) == 1
    assert loss(2, lv, 0, 4, 0.2, p, None) == 1 and loss(2, lv, 16, -1, 0.2, p, None) == 1
    for field in ("color", "target_color", "g_color", "depth"):
        keep = getattr(lv[1], field)
        setattr(lv[1], field, None)
        assert loss(2, lv, 16, 4, 0.2, p, None) == 1, field
        setattr(lv[1], field, keep)
    step = lib.splatraster_pose_step_window

    def sargs(n=2, dv=p, dp=p, w2c=p, pm=p, adv=1, state=p, view=p, proj=p):
        return (n, dv, dp, None, w2c, pm, 2e-3, 3e-3, 0.9, 0.999, 1e-8, adv, state, view, proj, None, None)
    for n in (0, -1, 9):
        assert step(*sargs(n=n)) == 1
    for k in ("w2c", "pm", "state", "view", "proj", "dv", "dp"):
        assert step(*sargs(**{k: None})) == 1, k
    assert all(x == 7.0 for x in cell)


def _inputs(N=3, Cn=3, H=6, W=8, P=5):
    g = dict(means3D=torch.zeros(P, 3), colors=torch.zeros(P, Cn), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 3),
             rotations=torch.zeros(P, 4))
    cam = SimpleNamespace(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, projection_matrix=torch.eye(4))
    return (torch.zeros(N, Cn, H, W), torch.zeros(N, 1, H, W)), g, cam, torch.eye(4).repeat(N, 1, 1)


def test_refine_poses_argument_errors_come_before_any_device_access():
    (c, d), g, cam, W0 = _inputs()
    with pytest.raises(ValueError, match="N == 0"):
        pose.refine_poses((c[:0], None), g, cam, W0[:0])
    with pytest.raises(ValueError, match="one \\[N,C,H,W\\] tensor"):
        pose.refine_poses((c[0], d[0]), g, cam, W0[0])
    with pytest.raises(ValueError, match="render_targets is"):
        pose.refine_poses(c, g, cam, W0[:1])
    with pytest.raises(ValueError, match="the camera 6x8"):
        pose.refine_poses((c[..., :7], None), g, cam, W0)
    with pytest.raises(ValueError, match="colour columns"):
        pose.refine_poses((c[:, :2], None), g, cam, W0)
    with pytest.raises(ValueError, match="for some frames only|depth targets for 2 of 3"):
        pose.refine_poses((c, d[:2]), g, cam, W0)
    with pytest.raises(ValueError, match="for some frames only"):
        pose.refine_poses((c, [d[0], None, d[2]]), g, cam, W0)
    with pytest.raises(ValueError, match="depth target is"):
        pose.refine_poses((c, d[..., :7]), g, cam, W0)
    with pytest.raises(ValueError, match="one start pose per frame"):
        pose.refine_poses((c, d), g, cam, W0[:2])
    with pytest.raises(ValueError, match="one start pose per frame"):
        pose.refine_poses((c, d), g, cam, W0[:, :3])
    with pytest.raises(ValueError, match="window >= 1"):
        pose.refine_poses((c, d), g, cam, W0, window=0)
    with pytest.raises(ValueError, match="iterations >= 0"):
        pose.refine_poses((c, d), g, cam, W0, iterations=-1)


def test_chunking_arithmetic():
    assert pose.window_chunk(6000, 8) == 8 and pose.window_chunk(6000, 100) == 8 and pose.window_chunk(6000, 5) == 5
    assert pose.window_chunk(6000, 1) == 1
    K = pose.window_chunk(500_000, 8)
    assert [min(K, 11 - a) for a in range(0, 11, K)] == [8, 3]                   # N = 11, window 8
    assert pose.window_chunk((1 << 24) // 8, 8) == 8
    assert pose.window_chunk((1 << 24) // 8 + 1, 8) == 7                         # P just above 2^24 / 8: 24-bit row ids
    assert pose.window_chunk((1 << 24) // 2 + 1, 8) == 1 and pose.window_chunk(1 << 25, 8) == 1
    assert pose.window_chunk(0, 8) == 8
