"""Host-side checks of the joint window backward (csrc/window_joint_bwd.hip, splatraster_backward_window_joint,
rasterizer.window_backward(cameras=True), pose.WindowPoses): the entry point is declared and bound with the header's argument
count, every argument error is returned before any device work, and the Python argument errors come before any device access."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from splatloc_amd import _native, pose, rasterizer

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "splatraster.h")
NAME = "splatraster_backward_window_joint"


def test_symbol_is_exported_declared_and_bound_with_the_headers_argument_count():
    text = open(HEADER).read()
    lib = _native.load()
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", text, re.S)
    assert m, "not declared"
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    n_args = len([a for a in decl.split(",") if a.strip()])
    assert n_args == 25
    assert NAME in _native.SYMBOLS and len(_native.SYMBOLS[NAME][1]) == n_args
    fn = getattr(lib, NAME)                                                      # exported
    assert fn.argtypes == _native.SYMBOLS[NAME][1] and fn.restype is C.c_int
    assert _native.ABI_VERSION == 20 and lib.splatraster_abi_version() == 20     # a new symbol only


def _host_ptr():
    """host memory: a launch or a memset on it would fault, an argument check returns first"""
    cell = (C.c_float * 64)(*([7.0] * 64))
    return cell, C.cast(cell, C.c_void_p)


def test_bad_arguments_return_before_any_launch():
    lib = _native.load()
    cell, p = _host_ptr()
    st = _native.Settings(48, 64, 1.0, 1.0, 1.0, 0, 0, 4, 0, 0, 0)
    views = (_native.WindowView * 8)()
    for w in views:
        w.viewmatrix = w.projmatrix = w.radii = w.out_color = w.out_depth = w.out_alpha = w.dL_dout_color = w.dL_dmeans2D = p.value
        w.tanfovx = w.tanfovy = 1.0
    R = (C.c_int64 * 8)(*([5] * 8))
    call = getattr(lib, NAME)

    def args(s=C.byref(st), V=2, vw=views, P=10, R_=R, m3=p, col=p, sca=p, rot=p, cov=None, geom=p, binning=p, img=p, dm3=p, dcol=p,
             dop=p, dsca=p, drot=p, dcov=None, ws=p, dv=p, dp=p):
        return (s, V, vw, P, R_, None, m3, col, sca, rot, cov, geom, binning, img, dm3, dcol, dop, dsca, drot, dcov, ws, dv, dp,
                None, None)
    for V in (0, 9, -3):
        assert call(*args(V=V)) == 1
    assert call(*args(s=None)) == 1 and call(*args(vw=None)) == 1 and call(*args(R_=None)) == 1 and call(*args(P=-1)) == 1
    assert call(*args(ws=None)) == 1 and call(*args(dv=None)) == 1 and call(*args(dp=None)) == 1
    assert call(*args(ws=None, P=0)) == 1 and call(*args(dv=None, P=0)) == 1      # also when there is nothing to differentiate
    assert call(*args(dm3=None)) == 1
    for k in ("m3", "col", "geom", "binning", "img", "sca", "rot", "dcol", "dop", "dsca", "drot"):
        assert call(*args(**{k: None})) == 1, k
    assert call(*args(cov=p, dcov=p)) == 1                                       # scales + rotations AND a covariance
    assert call(*args(cov=p, sca=None, rot=None, dcov=None)) == 1                # a covariance without its gradient
    Rn = (C.c_int64 * 8)(5, -1, 5, 5, 5, 5, 5, 5)
    assert call(*args(R_=Rn)) == 1
    for field in ("viewmatrix", "projmatrix", "radii", "out_color", "out_depth", "dL_dout_color", "dL_dmeans2D"):
        keep = getattr(views[1], field)
        setattr(views[1], field, None)
        assert call(*args()) == 1, field
        setattr(views[1], field, keep)
    views[1].color_grad_channels = 9                                             # more gradient planes than channels
    assert call(*args()) == 1
    views[1].color_grad_channels = 0
    assert all(x == 7.0 for x in cell)


def test_cameras_with_raw_raises_without_touching_the_device():
    f = SimpleNamespace()          # no attribute is read before the check
    with pytest.raises(ValueError, match="raw"):
        rasterizer.window_backward(f, [], cameras=True, raw=(None,) * 5)


def test_window_poses_argument_errors_come_before_any_device_access():
    eye = torch.eye(4)
    with pytest.raises(ValueError, match=r"\[N,4,4\]"):
        pose.WindowPoses(eye, eye)
    with pytest.raises(ValueError, match=r"\[N,4,4\]"):
        pose.WindowPoses(eye.repeat(0, 1, 1), eye)
    with pytest.raises(ValueError, match="projection_matrix"):
        pose.WindowPoses(eye.repeat(3, 1, 1), torch.eye(3))
    with pytest.raises(ValueError, match="fixed"):
        pose.WindowPoses(eye.repeat(3, 1, 1), eye, fixed=[3])
    with pytest.raises(RuntimeError, match="GPU"):
        pose.WindowPoses(eye.repeat(3, 1, 1), eye)      # a CPU tensor: no CPU fallback
