"""Where the compositing backward takes its dL/dout planes from, and when a quadrant leaves before loading them
(composite_bwd.hip: the set-up of every quadrant wave) — needs an MI355X.

The contract of a launch: colour planes [0, gc) behind dL_dcolor, channel C - 1 behind dL_dlast when gc < C, nothing in
between; s_end = bg . g over the background's entries.  Which channel of which pass reads what is decided per wave by scalar
compares with one form per case — every channel plain, all but the last, a few leading ones — and the background dot has a
short form for up to four entries and a general one.  Every case is driven through rasterize_window on the smallest frame
that has them all: 40x24 pixels = 3x2 tiles with a partial right column and bottom row and quadrants wholly outside the
image, 300 Gaussians, tile lists of 62-175 entries (checked below), 1 and 2 views, and the layouts
    C = 35 (the headline kernel), 36 (32 + 4; the headline kernel alone when the last channel has no gradient),
        32, 40 (32 + 8: a pass with c0 = 32), 4 (the narrow kernels).

Check A: every gradient against the CPU oracle, which gets the equivalent full [C,H,W] gradient with zero planes:
    helpers.assert_grad_close at its default bar for every tensor, helpers.assert_grad_rows_close at its default bar for
    every tensor with more than one column (on the one-column opacity rows that bar is a purely relative one on a signed,
    cancelling sum — helpers.py — which no test of the project bounds).  A colour column without a gradient has a reference
    row entry of exactly zero and must come back as exactly zero.
Check B: in the deterministic mode every split configuration is BIT-IDENTICAL to the same loss written as one full
    [C,H,W] gradient with explicit zero planes (split_last = False): both load the same values and differ only in the path
    that selects their source.
"""
import functools

import numpy as np
import pytest
import torch

from splatloc_amd.camera import PinholeCamera
from splatloc_amd.synthetic import make_scene
from tests.helpers import assert_grad_close, assert_grad_rows_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, P = 40, 24, 300
SCALE_MEDIAN = 0.15
LAYOUTS = (35, 36, 32, 40, 4)
BACKGROUNDS = ("zeros3", "random3", "many")
CONFIGS = ("full", "split_last_in_loss", "split_last_not_in_loss", "split_head3", "no_depth_alpha", "split_last_mixed")
NAMES = (("dL_dmeans3D", "means3D"), ("dL_dcolors", "colors"), ("dL_dopacities", "opac"), ("dL_dscales", "scales"),
         ("dL_drotations", "rots"))


def _background(kind, C):
    if kind == "zeros3":
        return torch.zeros(3)
    g = torch.Generator().manual_seed(99)
    # "many": an entry for every channel (six at C = 4) — more than four entries: the general form of the background dot,
    # with entries in the second pass of C = 40
    return torch.rand(3 if kind == "random3" else max(C, 6), generator=g)


@functools.lru_cache(maxsize=None)
def _scene(C, bg_kind, w=W, h=H, left_half=False):
    sc = make_scene(P, w, h, C, seed=7, scale_median=SCALE_MEDIAN)
    if left_half:   # every Gaussian well inside the left half of the frame
        cam = sc.camera
        z = sc.means3D[:, 2]
        sc.means3D[:, 0] = -(0.55 + 0.5 * torch.rand(P, generator=torch.Generator().manual_seed(3))) * z * cam.tanfovx
        sc.scales.mul_(0.2)
    sc.bg = _background(bg_kind, C)
    return sc


def _camera(sc, k):
    """view k of a window (view 0 = the scene's own camera) and its dL/dout planes"""
    cam0 = sc.camera
    ang = 0.03 * k
    R = torch.tensor([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], dtype=torch.float32)
    cam = PinholeCamera(cam0.image_width, cam0.image_height, cam0.fx * (1.0 + 0.02 * k), cam0.fy, cam0.cx + 0.5 * k,
                        cam0.cy - 0.25 * k, R, torch.tensor([0.02 * k, -0.01 * k, 0.05 * k]))
    g = tuple(torch.roll(t, shifts=11 * k, dims=-1).contiguous() for t in (sc.dL_dcolor, sc.dL_ddepth, sc.dL_dalpha))
    return cam, g


@functools.lru_cache(maxsize=None)
def _oracle_forward(C, bg_kind, k, w=W, h=H, left_half=False):
    from oracle import oracle
    sc = _scene(C, bg_kind, w, h, left_half)
    cam, _ = _camera(sc, k)
    return oracle.forward(oracle.Settings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy), sc.bg.numpy(),
                          sc.means3D.numpy(), sc.opacities.numpy(), cam.world_view_transform.numpy(),
                          cam.full_proj_transform.numpy(), cam.camera_center.numpy(), colors_precomp=sc.features.numpy(),
                          scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), omp=True)


def _plan(config, C, k):
    """(split_last argument, last channel in the loss, colour planes in the loss, depth / alpha in the loss) of view k"""
    if config == "full":
        return False, True, C, True
    if config == "split_last_in_loss":
        return True, True, C - 1, True
    if config == "split_last_not_in_loss":
        return True, False, C - 1, True
    if config == "split_head3":
        return 3, True, 3, True
    if config == "no_depth_alpha":
        return False, True, C, False
    if config == "split_last_mixed":      # view 0 has the last channel in its loss, view 1 has not
        return True, k == 0, C - 1, True
    raise ValueError(config)


def _equivalent_gradient(config, C, k, g):
    """the full [C,H,W] gradient (zero planes where the loss has none) that view k's loss amounts to"""
    _, last_in, head, _ = _plan(config, C, k)
    full = g.clone()
    full[head:C - 1] = 0.0
    if not last_in:
        full[C - 1] = 0.0
    return full


def _run(sc, V, config, explicit):
    """gradients of the window's loss; explicit = the same loss as full [C,H,W] gradients with zero planes, split_last = False"""
    from splatloc_amd import GaussianRasterizationSettings, rasterize_window
    C = sc.features.shape[1]
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    L = dict(means3D=leaf(sc.means3D), colors=leaf(sc.features), opac=leaf(sc.opacities), scales=leaf(sc.scales),
             rots=leaf(sc.rotations))
    cams = [_camera(sc, k) for k in range(V)]
    rss = []
    for cam, _ in cams:
        cam = cam.to(DEV)
        rss.append(GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, sc.bg.to(DEV), 1.0,
                                                 cam.world_view_transform, cam.full_proj_transform, 0, cam.camera_center,
                                                 False, False))
    m2s = [torch.zeros_like(L["means3D"], requires_grad=True) for _ in range(V)]
    split = False if explicit else _plan(config, C, 0)[0]
    outs = rasterize_window(rss, L["means3D"], m2s, L["colors"], L["opac"], scales=L["scales"], rotations=L["rots"],
                            split_last=split)
    loss = 0
    for k, (o, (_, g)) in enumerate(zip(outs, cams)):
        _, last_in, head, aux = _plan(config, C, k)
        gc_, gd_, ga_ = (t.to(DEV) for t in g)
        if explicit or not split:
            img, depth, alpha = o[0], o[1], o[2]
            loss = loss + (img * _equivalent_gradient(config, C, k, g[0]).to(DEV)).sum()
        else:
            rgb, last, depth, alpha = o[0], o[1], o[2], o[3]
            loss = loss + (rgb * gc_[:head]).sum()
            if last_in:
                loss = loss + (last * gc_[C - 1]).sum()
        if aux:
            loss = loss + (depth * gd_).sum() + (alpha * ga_).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = {nm: L[nm].grad.detach().clone() for _, nm in NAMES}
    for k, m in enumerate(m2s):
        res[f"means2D[{k}]"] = m.grad.detach().clone()
    return res


def _check_against_oracle(tag, sc, V, config, got, bg_kind, w=W, h=H, left_half=False):
    from oracle import oracle
    C = sc.features.shape[1]
    tot = {}
    for k in range(V):
        f = _oracle_forward(C, bg_kind, k, w, h, left_half)
        _, g = _camera(sc, k)
        aux = _plan(config, C, k)[3]
        b = oracle.backward(f, _equivalent_gradient(config, C, k, g[0]).numpy(), g[1].numpy() if aux else None,
                            g[2].numpy() if aux else None, omp=True)
        for key, _ in NAMES:
            tot[key] = b[key].astype(np.float64) + tot.get(key, 0.0)
        m2 = got[f"means2D[{k}]"].cpu().numpy()
        assert_grad_close(f"{tag} means2D[{k}]", m2, b["dL_dmeans2D"])
        assert_grad_rows_close(f"{tag} rows means2D[{k}]", m2, b["dL_dmeans2D"])
    for key, nm in NAMES:
        a = got[nm].cpu().numpy()
        assert_grad_close(f"{tag} {key}", a, tot[key])
        if a.reshape(a.shape[0], -1).shape[1] > 1:
            assert_grad_rows_close(f"{tag} rows {key}", a, tot[key])


def test_the_scene_has_the_lists_the_cases_need():
    """tile lists of roughly 50-200 entries in every tile of both views (more than one 64-entry chunk, several staging
    rounds), counted on the CPU oracle"""
    for k in range(2):
        r = np.asarray(_oracle_forward(35, "zeros3", k)["ranges"]).reshape(-1, 2)
        n = r[:, 1].astype(np.int64) - r[:, 0].astype(np.int64)
        assert n.shape[0] == 6 and n.min() >= 50 and n.max() <= 200, n


def _configs(C, V):
    return [c for c in CONFIGS if V == 2 or c != "split_last_mixed"]


@pytest.mark.parametrize("V", (1, 2))
@pytest.mark.parametrize("bg_kind", BACKGROUNDS)
@pytest.mark.parametrize("C", LAYOUTS)
def test_every_source_layout_against_the_oracle(C, bg_kind, V):
    """Check A for every gradient configuration of the layout"""
    sc = _scene(C, bg_kind)
    for config in _configs(C, V):
        got = _run(sc, V, config, explicit=False)
        _check_against_oracle(f"C={C} {bg_kind} V={V} {config}", sc, V, config, got, bg_kind)


@pytest.mark.parametrize("V", (1, 2))
@pytest.mark.parametrize("bg_kind", BACKGROUNDS)
@pytest.mark.parametrize("C", LAYOUTS)
def test_split_sources_equal_explicit_zero_planes_bit_for_bit(C, bg_kind, V):
    """Check B for every split configuration of the layout"""
    from splatloc_amd import _native
    sc = _scene(C, bg_kind)
    _native.set_deterministic(True)
    try:
        for config in _configs(C, V):
            if not config.startswith("split"):
                continue
            a = _run(sc, V, config, explicit=False)
            b = _run(sc, V, config, explicit=True)
            for nm in a:
                diff = (a[nm] != b[nm])
                assert torch.equal(a[nm], b[nm]), (f"C={C} {bg_kind} V={V} {config}: {nm} differs in {int(diff.sum())} of "
                                                   f"{diff.numel()} elements, worst |d| {float((a[nm] - b[nm]).abs().max()):.3e} "
                                                   f"at scale {float(b[nm].abs().max()):.3e}")
    finally:
        _native.set_deterministic(False)


@pytest.mark.parametrize("C", (35, 4))
def test_quadrants_without_work_leave_early(C):
    """Check A where most waves return before their set-up: Gaussians in the left half of the frame only (the right column's
    tiles have empty lists), and an 8x8 frame (one quadrant inside the image, three outside)"""
    sc = _scene(C, "random3", W, H, True)
    r = np.asarray(_oracle_forward(C, "random3", 0, W, H, True)["ranges"]).reshape(-1, 2)
    n = (r[:, 1].astype(np.int64) - r[:, 0].astype(np.int64)).reshape(2, 3)
    assert (n[:, 2] == 0).all() and (n[:, 0] > 0).all(), n
    for config in ("full", "split_head3"):
        got = _run(sc, 1, config, explicit=False)
        _check_against_oracle(f"C={C} left half {config}", sc, 1, config, got, "random3", W, H, True)
    sc = _scene(C, "random3", 8, 8)
    for config in ("full", "split_head3"):
        got = _run(sc, 1, config, explicit=False)
        _check_against_oracle(f"C={C} 8x8 {config}", sc, 1, config, got, "random3", 8, 8)
