"""The bounded window forward (splatraster_forward_window_bounded, rasterizer.window_forward(bounded=...)) against the two-stage
forward of the same frame — needs an MI355X.

A frame that fits the caller's capacity must be bit-identical to the two-stage forward (outputs, point list, range table,
n_contrib, final_T); a frame that does not fit must render the background, leave an all-zero range table, touch no per-instance
element of `binning` and nothing behind it, record itself in the status block and give an all-zero backward; the flag is sticky
until the block is cleared.  64x48 frames (4x3 tiles) of 300 Gaussians, one and three views; the long-list tiers of the per-tile
sort on a 32x32 frame."""
import ctypes as C

import pytest
import torch

from splatloc_amd import _native, introspect
from splatloc_amd.rasterizer import BoundedWindow, window_backward, window_forward
from splatloc_amd.synthetic import make_scene
from tests.test_gpu_binsort import _concentrate
from tests.test_gpu_window import _views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0xA5
PAD = 4096


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    _native.set_front_end(-1)
    _native.check(_native.load().splatraster_debug_set_tile_sort_cap(0), "tile_sort_cap")


def _scene(P=300, W=64, H=48, seed=5, scale_median=0.08):
    sc = make_scene(P, W, H, 4, seed, scale_median=scale_median)
    sc.bg = torch.tensor([0.25, 0.5, 0.75])
    return sc


def _settings(sc, V):
    return [rs for _cam, rs, _g in _views(sc, V, torch.device(DEV))]


def _forward(sc, settings, bounded=None):
    dev = torch.device(DEV)
    return window_forward(sc.means3D.to(dev), sc.features.to(dev), sc.opacities.to(dev), sc.scales.to(dev), sc.rotations.to(dev),
                          None, settings, bounded=bounded)


def _layouts(f, n):
    """Byte spans of a window frame's binning buffer laid out for n instances (splatloc_amd.introspect.binning_spans): the four
    list arrays fill [0, ranges), then the range table, then (further back) the payload arrays irec | ipack; `total`: its size."""
    W, H = f.st.image_width, f.st.image_height
    L = introspect.binning_spans(f.V, n, W, H)
    L["lists_end"] = L["ranges"]
    L["total"] = _native.load().splatraster_window_binning_bytes(f.P, f.V, n, W, H, f.st.channels)
    return L


def _words(buf, off, count):
    return buf[off:off + 4 * count].view(torch.int32)


def _assert_same_frame(fb, ft, capacity):
    """bounded frame fb == two-stage frame ft, bit for bit"""
    R = sum(ft.R)
    for k in ("color", "depth", "alpha"):
        assert torch.equal(getattr(fb, k).view(torch.int32), getattr(ft, k).view(torch.int32)), k
    assert torch.equal(fb.radii, ft.radii)
    Lb, Lt = _layouts(fb, capacity), _layouts(ft, R)
    assert torch.equal(_words(fb.binning, Lb["point_list"], R), _words(ft.binning, Lt["point_list"], R)), "point_list"
    assert torch.equal(_words(fb.binning, Lb["ranges"], 2 * Lb["tiles"]), _words(ft.binning, Lt["ranges"], 2 * Lt["tiles"])), "ranges"
    IL = _native.ImageLayout()
    _native.check(_native.load().splatraster_get_window_image_layout(fb.st.image_width, fb.st.image_height, fb.V, C.byref(IL)), "layout")
    npix = fb.V * fb.st.image_width * fb.st.image_height
    assert torch.equal(_words(fb.img, IL.final_T, npix), _words(ft.img, IL.final_T, npix)), "final_T bits"
    assert torch.equal(_words(fb.img, IL.n_contrib, npix), _words(ft.img, IL.n_contrib, npix)), "n_contrib"


def _background_frame(sc, settings):
    """what a frame without instances looks like: the two-stage forward of the scene moved behind the camera"""
    z = sc.means3D.clone()
    sc.means3D[:, 2] = -1.0
    try:
        f = _forward(sc, settings)
        assert sum(f.R) == 0
        return f
    finally:
        sc.means3D.copy_(z)


def _assert_overflowed(fb, bw, bgf, R, tag):
    torch.cuda.synchronize()
    s = bw.status.read()
    assert (s.overflow, s.first_total, s.first_tag, s.total) == (1, R, tag, R)
    for k in ("color", "depth", "alpha"):
        assert torch.equal(getattr(fb, k).view(torch.int32), getattr(bgf, k).view(torch.int32)), k + " is not the background"
    L = _layouts(fb, bw.capacity)
    buf = bw.binning
    assert buf.numel() == L["total"] + PAD
    assert int(_words(buf, L["ranges"], 2 * L["tiles"]).abs().max()) == 0, "range table"
    assert bool((buf[:L["lists_end"]] == PATTERN).all()), "a list array was written"
    assert bool((buf[L["irec"]:L["payload_end"]] == PATTERN).all()), "a payload array was written"
    assert bool((buf[L["total"]:] == PATTERN).all()), "the bytes behind the buffer were written"


_OPEN = []


@pytest.fixture(autouse=True, scope="module")
def _close_status_blocks():
    yield
    torch.cuda.synchronize()
    for bw in _OPEN:
        bw.close()
    _OPEN.clear()


def _window(capacity, P, V, W, H, status=None):
    """a bounded window whose buffer is PAD bytes longer than the layout and pre-filled with the pattern"""
    bw = BoundedWindow(torch.device(DEV), capacity, status=status)
    n = bw.reserve(capacity, P, V, W, H, 4).numel()
    bw.binning = torch.full((n + PAD,), PATTERN, dtype=torch.uint8, device=DEV)
    _OPEN.append(bw)
    return bw


def _zero_backward(sc, f, V):
    dev = torch.device(DEV)
    grads = [(g[0], None, g[1], g[2]) for _cam, _rs, g in _views(sc, V, dev)]
    d = window_backward(f, grads)
    torch.cuda.synchronize()
    assert float(d["flat"].abs().max()) == 0.0 and float(d["m2"].abs().max()) == 0.0      # (NaN fails the comparison)


@pytest.fixture(scope="module")
def frames():
    """scene, settings, the two-stage frame and the background frame per view count: computed once, never modified"""
    out = {}
    for V in (1, 3):
        sc = _scene()
        settings = _settings(sc, V)
        out[V] = (sc, settings, _forward(sc, settings), _background_frame(sc, settings))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("extra", [0, 1000])
def test_a_frame_that_fits_equals_the_two_stage_forward(frames, V, extra):
    sc, settings, ft, _bg = frames[V]
    R = sum(ft.R)
    assert R > 0
    bw = _window(R + extra, ft.P, V, 64, 48)
    bw.next_tag = 11
    fb = _forward(sc, settings, bounded=bw)
    assert fb.R is None and fb.capacity == R + extra and bw.next_tag == 12
    torch.cuda.synchronize()
    _assert_same_frame(fb, ft, R + extra)
    s = bw.status.read()
    assert (s.total, s.overflow, s.last_tag) == (R, 0, 11)
    assert bool((bw.binning[_layouts(fb, R + extra)["total"]:] == PATTERN).all())


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("capacity", ["R-1", "0"])
def test_a_frame_that_does_not_fit_renders_background_writes_nothing_and_is_sticky(frames, V, capacity):
    sc, settings, ft, bgf = frames[V]
    R = sum(ft.R)
    bw = _window(R - 1 if capacity == "R-1" else 0, ft.P, V, 64, 48)
    bw.next_tag = 41
    fb = _forward(sc, settings, bounded=bw)
    _assert_overflowed(fb, bw, bgf, R, 41)
    _zero_backward(sc, fb, V)
    # sticky: ample capacity and a new tag, the same status block
    big = _window(R + 1000, ft.P, V, 64, 48, status=bw.status)
    big.next_tag = 42
    f2 = _forward(sc, settings, bounded=big)
    torch.cuda.synchronize()
    s = bw.status.read()
    assert (s.overflow, s.first_tag, s.first_total, s.last_tag, s.total) == (1, 41, R, 42, R)
    for k in ("color", "depth", "alpha"):
        assert torch.equal(getattr(f2, k).view(torch.int32), getattr(bgf, k).view(torch.int32)), k
    L = _layouts(f2, R + 1000)
    assert bool((big.binning[:L["lists_end"]] == PATTERN).all()) and bool((big.binning[L["irec"]:L["payload_end"]] == PATTERN).all())
    # cleared: the same call now renders the frame
    bw.status.clear()
    f3 = _forward(sc, settings, bounded=big)
    torch.cuda.synchronize()
    _assert_same_frame(f3, ft, R + 1000)
    s = bw.status.read()
    assert (s.overflow, s.total, s.last_tag) == (0, R, 43)


def test_an_empty_frame_renders_background_without_overflow(frames):
    sc, settings, _ft, bgf = frames[1]
    z = sc.means3D.clone()
    sc.means3D[:, 2] = -1.0          # every Gaussian behind the camera
    try:
        bw = _window(4096, 300, 1, 64, 48)
        fb = _forward(sc, settings, bounded=bw)
        torch.cuda.synchronize()
    finally:
        sc.means3D.copy_(z)
    s = bw.status.read()
    assert (s.overflow, s.total) == (0, 0)
    _assert_same_frame(fb, bgf, 4096)
    assert int(_words(bw.binning, _layouts(fb, 4096)["ranges"], 24).abs().max()) == 0
    _zero_backward(sc, fb, 1)


@pytest.mark.parametrize("n,cap", [(2500, 4096), (5000, 0)])
def test_long_lists_fit_or_overflow_like_short_ones(n, cap):
    """One tile of a 32x32 frame holds n entries: 2 500 are the wide instantiation's of the per-tile launch (forced), 5 000 the
    long-list launch's."""
    _native.set_front_end(1)
    _native.check(_native.load().splatraster_debug_set_tile_sort_cap(cap), "tile_sort_cap")
    sc = _concentrate(_scene(n, 32, 32, seed=9, scale_median=0.02), n, (8.3, 7.6))
    settings = _settings(sc, 1)
    ft = _forward(sc, settings)
    R = sum(ft.R)
    L = _layouts(ft, R)
    rng = _words(ft.binning, L["ranges"], 2 * L["tiles"]).view(-1, 2).long()
    longest = int((rng[:, 1] - rng[:, 0]).max())
    assert (2048 < longest <= 4096) if n == 2500 else (4096 < longest <= 16384), longest
    bgf = _background_frame(sc, settings)
    bw = _window(R, n, 1, 32, 32)
    fb = _forward(sc, settings, bounded=bw)
    torch.cuda.synchronize()
    _assert_same_frame(fb, ft, R)
    s = bw.status.read()
    assert (s.total, s.overflow) == (R, 0)
    small = _window(R - 1, n, 1, 32, 32)
    small.next_tag = 5
    fo = _forward(sc, settings, bounded=small)
    _assert_overflowed(fo, small, bgf, R, 5)
    _zero_backward(sc, fo, 1)


def test_the_radix_front_end_is_unsupported_and_launches_nothing(frames):
    sc, settings, ft, _bg = frames[1]
    _native.set_front_end(0)         # the frame shape no longer selects the binned front end
    bw = _window(sum(ft.R) + 10, ft.P, 1, 64, 48)
    bw.next_tag = 77
    with pytest.raises(RuntimeError, match="unsupported"):
        _forward(sc, settings, bounded=bw)
    torch.cuda.synchronize()
    s = bw.status.read()
    assert (s.total, s.overflow, s.last_tag) == (0, 0, 0)
    assert bool((bw.binning == PATTERN).all())
