"""The backward's gradient accumulator for wide feature tables (C >= 32; csrc/common.h, GaccLayout): the dL/dfeature columns
that fill whole 64-byte lines are ONE row per Gaussian into which all views of a window add (the float atomics form the sum
over the views), only the line with the tail colours and the 7 moments is per (view, Gaussian) — needs an MI355X.

Through rasterize_window (the window C ABI): summed parameter gradients against the sum of the CPU oracle's per-view gradients
and against V per-view calls, the deterministic mode, the chunked channel passes (C = 40, 48: columns from 32 on arrive in
narrow launches), and the accumulator's own contents for views that do not see the scene."""
import numpy as np
import pytest
import torch

from splatloc_amd.camera import PinholeCamera
from splatloc_amd.synthetic import make_scene
from tests.helpers import assert_grad_close
from tests.test_gpu_window import FULL_TENSOR, _leaves, _serial, _window

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = (("dL_dmeans3D", "means3D"), ("dL_dcolors", "colors"), ("dL_dopacities", "opac"), ("dL_dscales", "scales"),
         ("dL_drotations", "rots"))


def _views(sc, V, dev, away=()):
    """V cameras around the scene's own (test_gpu_window._views); the ones listed in `away` look the other way"""
    from splatloc_amd import GaussianRasterizationSettings
    cam0 = sc.camera
    W, H = cam0.image_width, cam0.image_height
    out = []
    for k in range(V):
        ang = 0.03 * (k - V // 2) + (np.pi if k in away else 0.0)
        R = torch.tensor([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], dtype=torch.float32)
        cam = PinholeCamera(W, H, cam0.fx * (1.0 + 0.02 * k), cam0.fy, cam0.cx + 0.5 * k, cam0.cy - 0.25 * k, R,
                            torch.tensor([0.02 * k, -0.01 * k, 0.05 * k])).to(dev)
        rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, sc.bg.to(dev), 1.0, cam.world_view_transform,
                                           cam.full_proj_transform, 0, cam.camera_center, False, False)
        g = tuple(torch.roll(t, shifts=11 * k + 1, dims=-1).contiguous().to(dev) for t in (sc.dL_dcolor, sc.dL_ddepth, sc.dL_dalpha))
        out.append((cam, rs, g))
    return out


def _oracle(sc, views):
    """sum over the views of the oracle's parameter gradients (float64), and its dL/dmeans2D per view"""
    from oracle import oracle
    tot, m2 = {}, []
    for cam, rs, g in views:
        f = oracle.forward(oracle.Settings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy), sc.bg.numpy(),
                           sc.means3D.numpy(), sc.opacities.numpy(), cam.world_view_transform.cpu().numpy(),
                           cam.full_proj_transform.cpu().numpy(), cam.camera_center.cpu().numpy(),
                           colors_precomp=sc.features.numpy(), scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), omp=True)
        b = oracle.backward(f, g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy(), omp=True)
        for k, _ in NAMES:
            tot[k] = b[k].astype(np.float64) + tot.get(k, 0.0)
        m2.append((b["dL_dmeans2D"], f["radii"]))
    return tot, m2


def _check_window(sc, V, bars=None, away=()):
    bars = bars or {}
    dev = torch.device(DEV)
    views = _views(sc, V, dev, away)
    tot, m2o = _oracle(sc, views)
    Lw, outs, m2w, _ = _window(sc, views, dev)
    for v in range(V):
        assert_grad_close(f"means2D[{v}]", m2w[v].grad.cpu().numpy(), m2o[v][0], **bars)
    for k, nm in NAMES:
        assert_grad_close(k, Lw[nm].grad.cpu().numpy(), tot[k], **bars)
    return views, Lw, m2w, tot, m2o


def _check_against_per_view_calls(sc, views, Lw, m2w):
    Ls, _, m2s, _ = _serial(sc, views, torch.device(DEV))
    for v in range(len(views)):
        assert_grad_close(f"means2D[{v}] vs per-view call", m2w[v].grad.cpu().numpy(), m2s[v].grad.cpu().numpy())
    for _, nm in NAMES:
        assert_grad_close(f"{nm} vs per-view calls", Lw[nm].grad.cpu().numpy(), Ls[nm].grad.cpu().numpy())


@pytest.mark.parametrize("C", [35, 32])
@pytest.mark.parametrize("V", [1, 3, 5, 8])
def test_wide_window_against_oracle_and_per_view_calls(C, V):
    sc = make_scene(P=3000, W=208, H=144, C=C, seed=900 + 10 * C + V, scale_median=0.04)
    views, Lw, m2w, _, _ = _check_window(sc, V)
    _check_against_per_view_calls(sc, views, Lw, m2w)


@pytest.mark.parametrize("C", [40, 48])
@pytest.mark.parametrize("small_panel", [True, False])
def test_chunked_channel_passes_land_in_the_right_table(C, small_panel):
    """C = 40: 32 + 8 channels, the second launch's columns 32 .. 39 are per view; C = 48: 32 + 16, columns 32 .. 47 are shared.
    Small frames take the panel variant of the narrow launches (their flush addresses the columns), large ones the butterfly
    variant (its slots do): both are run on the same frame through the launch-selection hook."""
    from splatloc_amd import _native
    lib = _native.load()
    sc = make_scene(P=2500, W=176, H=128, C=C, seed=930 + C, scale_median=0.04)
    lib.splatraster_debug_set_small_panel_max_waves(-1 if small_panel else 0)
    try:
        views, Lw, m2w, _, _ = _check_window(sc, 3)
        _check_against_per_view_calls(sc, views, Lw, m2w)
    finally:
        lib.splatraster_debug_set_small_panel_max_waves(-1)


def test_deterministic_mode_uses_the_same_layout():
    """int64 fixed-point adds are associative: the shared rows stay bit-reproducible whatever the order in which the views'
    waves arrive; against the oracle with the deterministic bars of test_gpu_window (FULL_TENSOR)."""
    from splatloc_amd import _native
    sc = make_scene(P=3000, W=208, H=144, C=35, seed=951, scale_median=0.04)
    dev = torch.device(DEV)
    _native.set_deterministic(True)
    try:
        views, La, m2a, _, _ = _check_window(sc, 3, bars=FULL_TENSOR)
        Lb, _, m2b, _ = _window(sc, views, dev)
        for _, nm in NAMES:
            assert torch.equal(La[nm].grad, Lb[nm].grad), nm
        for a, b in zip(m2a, m2b):
            assert torch.equal(a.grad, b.grad)
    finally:
        _native.set_deterministic(False)


def _accumulator(binning, lib, P, V, R, W, H, C):
    """(shared [P, SH], per-view [V, P, PV]) views of the accumulator inside a window's `binning` buffer: it is followed by the
    camera-gradient sets, the (unused: C > 4) checkpoint section, the launch order and the part counts (csrc/capi.hip)"""
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    tiles = ((W + 15) // 16) * ((H + 15) // 16) * V
    SH = C & ~15
    mo = C if (C & 15) + 7 <= 16 else (C + 15) & ~15
    PV = ((mo + 7 + 15) & ~15) - SH
    nfl = P * SH + V * P * PV
    total = lib.splatraster_window_binning_bytes(P, V, R, W, H, C)
    assert binning.numel() >= total
    off = total - 2 * al(4 * tiles) - al(16) - (16 * 64 * 4 + 256) - al(4 * nfl)
    fl = binning[off:off + 4 * nfl].view(torch.float32)
    return fl[:P * SH].view(P, SH), fl[P * SH:].view(V, P, PV), SH, mo - SH


@pytest.mark.parametrize("C", [35, 40])
def test_views_that_do_not_see_a_gaussian_leave_their_lines_zero(C):
    """Two of five cameras look the other way.  The shared row of every Gaussian is the sum over the views that see it (the
    oracle's, whose gradient for the other views is exactly zero), and the per-view lines of the views that do not see it are
    still at the zero the buffer was cleared to."""
    from splatloc_amd import _native, introspect, rasterize_window
    lib = _native.load()
    P, W, H, V, away = 3000, 208, 144, 5, (1, 3)
    sc = make_scene(P=P, W=W, H=H, C=C, seed=960 + C, scale_median=0.04)
    dev = torch.device(DEV)
    views = _views(sc, V, dev, away)
    tot, m2o = _oracle(sc, views)
    for v in away:
        assert not m2o[v][1].any() and not m2o[v][0].any()          # nothing visible, no gradient
    L = _leaves(sc, dev)
    m2s = [torch.zeros_like(L["means3D"], requires_grad=True) for _ in views]
    outs = rasterize_window([rs for _, rs, _ in views], L["means3D"], m2s, L["colors"], L["opac"], scales=L["scales"],
                            rotations=L["rots"])
    fn = outs[0][0].grad_fn
    binning, R = introspect.forward_buffers(fn)[1], int(sum(fn.R))
    loss = 0
    for (color, depth, alpha, radii), (_, _, g) in zip(outs, views):
        loss = loss + (color * g[0]).sum() + (depth * g[1]).sum() + (alpha * g[2]).sum()
    loss.backward()
    torch.cuda.synchronize()
    for k, nm in NAMES:
        assert_grad_close(k, L[nm].grad.cpu().numpy(), tot[k])
    shared, per_view, SH, MO = _accumulator(binning, lib, P, V, R, W, H, C)
    dcol = L["colors"].grad
    assert torch.equal(shared, dcol[:, :SH])                         # the copy of the shared table, bit for bit
    tail = torch.zeros_like(dcol[:, SH:])
    for v in range(V):
        seen = outs[v][3] > 0
        assert float(per_view[v][~seen].abs().max()) == 0.0          # lines of (view, Gaussian) pairs the view does not see
        if v in away:
            assert not bool(seen.any()) and float(per_view[v].abs().max()) == 0.0
            assert float(m2s[v].grad.abs().max()) == 0.0
        else:
            assert float(per_view[v][:, MO:MO + 7].abs().max()) > 0.0
            tail = tail + torch.where(seen[:, None], per_view[v][:, :C - SH], torch.zeros_like(tail))
    assert torch.equal(tail, dcol[:, SH:])                           # tail colours: summed in view order by preprocess_bwd
    seen_any = torch.stack([outs[v][3] > 0 for v in range(V)]).any(0)
    assert float(shared[~seen_any].abs().max() if bool((~seen_any).any()) else 0.0) == 0.0
