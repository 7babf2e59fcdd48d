"""Host-side checks of the bounded window forward (include/splatraster.h "bounded window forward", csrc/bounded.hip,
rasterizer.BoundedWindow, training.refine_bounded): the new entry points are exported, declared and bound with the header's argument
counts, the ABI version did not move, argument errors come back before any device work, and the host half of the rewind — step
counts and learning rates — restores exactly what a snapshot held."""
import ctypes as C
import os
import re

import torch

from splatloc_amd import _native, training

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "splatraster.h")
NEW = {"splatraster_bounded_status_create": 1, "splatraster_bounded_status_destroy": 1, "splatraster_bounded_status_read": 2,
       "splatraster_bounded_status_clear": 2, "splatraster_forward_window_bounded_supported": 4,
       "splatraster_forward_window_bounded": 18, "splatraster_forward_window_bounded_raw": 14,
       "splatraster_adam_step_gated": 8, "splatraster_adam_step_radii_gated": 11}


def test_new_symbols_are_exported_declared_and_bound():
    text = open(HEADER).read()
    lib = _native.load()
    for name, n_expected in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert m, name + ": not declared"
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        n_args = len([a for a in decl.split(",") if a.strip()])
        assert n_args == n_expected, (name, n_args)
        assert name in _native.SYMBOLS and len(_native.SYMBOLS[name][1]) == n_args, name
        fn = getattr(lib, name)                                                  # exported
        assert fn.argtypes == _native.SYMBOLS[name][1] and fn.restype is C.c_int
    assert "typedef struct splatraster_bounded_status" in text
    assert C.sizeof(_native.BoundedStatus) == 64


def test_abi_version_is_still_20():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SPLATRASTER_ABI_VERSION\s+20\b", text)
    assert _native.ABI_VERSION == 20 and _native.load().splatraster_abi_version() == 20      # new symbols only


def test_argument_errors_return_before_any_device_work():
    lib = _native.load()
    cell = (C.c_float * 64)(*([7.0] * 64))      # host memory: a launch on it would fault, an argument check returns first
    p = C.cast(cell, C.c_void_p)
    st = _native.Settings(48, 64, 1.0, 1.0, 1.0, 0, 0, 4, 0, 0, 0)
    views = (_native.WindowView * 2)()
    for w in views:
        w.viewmatrix = w.projmatrix = w.radii = w.out_color = w.out_depth = w.out_alpha = p.value
        w.tanfovx = w.tanfovy = 1.0
    fake_status = (C.c_void_p * 4)(p.value, p.value, p.value, 0)     # a handle's shape: never dereferenced on these paths
    hs = C.cast(fake_status, C.c_void_p)

    def call(s=C.byref(st), V=1, P=10, status=hs, capacity=100, geom=p, binning=p, img=p, col=p):
        return lib.splatraster_forward_window_bounded(s, V, views, P, p, p, p, p, None, None, col, geom, binning, img, capacity, 3,
                                                      status, None)
    assert call(status=None) == 1 and call(capacity=-1) == 1 and call(V=0) == 1 and call(V=9) == 1 and call(s=None) == 1
    assert call(P=-1) == 1 and call(geom=None) == 1 and call(binning=None) == 1 and call(img=None) == 1 and call(col=None) == 1
    assert call(capacity=1 << 31) == 4                                   # more instances than a frame can have
    assert call(P=0) == _native.ERR_UNSUPPORTED                          # no front end runs on an empty model
    assert lib.splatraster_forward_window_bounded_raw(C.byref(st), 1, views, 10, p, None, None, p, p, p, 100, 0, hs, None) == 1
    assert lib.splatraster_bounded_status_read(None, None) == 1 and lib.splatraster_bounded_status_clear(None, None) == 1
    assert lib.splatraster_bounded_status_create(None) == 1 and lib.splatraster_bounded_status_destroy(None) == 0
    grp = (_native.AdamGroup * 1)()
    assert lib.splatraster_adam_step_gated(1, grp, 0.9, 0.999, 1e-15, 0.0, None, None) == 1
    assert lib.splatraster_adam_step_radii_gated(0, grp, 0.9, 0.999, 1e-15, 0.0, 4, p, p, None, None) == 1
    assert all(x == 7.0 for x in cell)


def test_supported_follows_the_front_end_choice():
    try:
        assert _native.bounded_supported(300, 1, 64, 48) and _native.bounded_supported(500_000, 1, 640, 480)
        assert not _native.bounded_supported(0, 1, 64, 48) and not _native.bounded_supported(300, 9, 64, 48)
        assert not _native.bounded_supported(500_000, 1, 1920, 1080)     # 8 160 lists: the radix front end's frame
        _native.set_front_end(0)
        assert not _native.bounded_supported(300, 1, 64, 48)
        _native.set_front_end(1)
        assert _native.bounded_supported(300, 1, 64, 48)
    finally:
        _native.set_front_end(-1)


def test_host_optimizer_state_snapshot_restores_steps_and_learning_rates():
    a, b = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    opt = torch.optim.Adam([{"params": [a], "lr": 0.1, "name": "xyz"}, {"params": [b], "lr": 0.2, "name": "f_dc"}])
    a.grad = torch.ones(3)
    opt.step()                                       # `a` has state (step 1), `b` has none yet
    snap = training._host_optimizer_state(opt)
    assert snap == [(0.1, [1.0]), (0.2, [None])]
    b.grad = torch.ones(2)
    for _ in range(3):
        opt.step()
    opt.param_groups[0]["lr"] = 0.05
    training._restore_host_optimizer_state(opt, snap)
    assert float(opt.state[a]["step"]) == 1.0 and float(opt.state[b]["step"]) == 0.0
    assert [g["lr"] for g in opt.param_groups] == [0.1, 0.2]
