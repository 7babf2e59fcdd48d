"""The forward's dead marks and the backward that honours them against tests/dead_marks_reference.py and the CPU
oracle — needs an MI355X.

The wide forward (C > 4) ORs bit 28 + q into the payload word of every list entry it evaluated for quadrant q with no lane live;
the backward skips those entries unless splatraster_debug_set_dead_marks(0) says otherwise.  Checked here, on the occluder scene
of the reference module (one tile list of ~190 entries: a near layer that finishes quadrants inside the first chunk, small
Gaussians behind it, pixel-missing Gaussians at every depth):

  * every marked (entry, quadrant) has its reach bit and is no contributor (`must_not`); every `must_mark` entry is marked where
    the kernel marks (C = 35, 36: the pass that writes the auxiliary planes; C = 3: the narrow walkers leave the stream unmarked);
  * ids, reach bits, ranges, n_contrib, final_T, the images and the marks themselves are bit-identical with the switch on and off;
  * gradients: torch.equal between on and off in the deterministic mode, the oracle bars of tests/test_gpu_parity.py otherwise;
  * a second forward over the same buffers leaves the same marks (the front end rewrites the stream in between: that the
    compositing forward itself reads bits 24..27 and the id only is what C = 36 shows, whose second channel pass walks the stream
    the first one marked; no entry point launches the compositing forward alone);
  * the backward skips exactly what is marked: with every entry marked by hand it walks nothing and every gradient is zero, with
    the switch off it ignores the same marks;
  * a render that no backward can follow (parameters under torch.no_grad(), or no input that requires a gradient) writes no marks;
  * the same as a window of two views with different cameras (row0 != 0), on frames with quadrants outside the image, and on the
    compact stream behind the radix front end.
"""
import functools

import numpy as np
import pytest
import torch

from splatloc_amd import _native, introspect
from tests.dead_marks_reference import SCENES, dead_mark_sets, occluder_scene
from tests.helpers import HipRun, assert_grad_close, oracle_backward, oracle_forward
from tests.test_gpu_parity import _check_backward, _check_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("means3D", "means2D", "opacities", "colors", "scales", "rotations")


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _native.set_dead_marks(True)
    _native.set_deterministic(False)
    _native.set_front_end(-1)


@functools.lru_cache(maxsize=None)
def _case(name, C):
    """the scene, the oracle's forward and backward of it: computed once, shared, never written to"""
    sc = occluder_scene(C, **SCENES[name])
    f = oracle_forward(sc)
    return sc, f, oracle_backward(f, sc)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _quads(x):
    """[n] words -> [n, 4] bool, bit q in column q"""
    return ((x.long()[:, None] >> torch.arange(4, device=x.device)[None]) & 1).bool().cpu().numpy()


def _full_stream(pay, ranges, R, compact):
    """reach bits and marks [R, 4] by FULL list position (a compact stream holds the live entries only: the others reach nothing)"""
    if not compact:
        assert pay["ids"].numel() == R
        return _quads(pay["imask"]), _quads(pay["idead"])
    cr = pay["cranges"].long()
    lens = cr[:, 1] - cr[:, 0]
    lst = torch.repeat_interleave(torch.arange(cr.shape[0], device=cr.device), lens)
    at = (ranges.long()[lst, 0] + pay["back"].long() - 1).cpu().numpy()
    reach, dead = np.zeros((R, 4), bool), np.zeros((R, 4), bool)
    reach[at], dead[at] = _quads(pay["imask"]), _quads(pay["idead"])
    return reach, dead


def _run(sc, marks, compact=False, backward=True):
    _native.set_dead_marks(marks)
    r = HipRun(sc, backward=False)
    cam = sc.camera
    st = introspect.payload_state(introspect.forward_buffers(r.color.grad_fn), r.num_rendered, cam.image_width, cam.image_height,
                                  compact=compact)
    r.payload = {k: v.clone() for k, v in st.items()}
    if backward:
        dev = r.color.device
        ((r.color * sc.dL_dcolor.to(dev)).sum() + (r.depth * sc.dL_ddepth.to(dev)).sum() + (r.alpha * sc.dL_dalpha.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return r


def _check_marks(reach, dead, f, W, H, marking, tag=""):
    """the marks of one view against the reference (the stream's own reach bits decide `walked`); returns the reference's sets"""
    s = dead_mark_sets(f, W, H, reach=reach)
    n_walked, n_dead = int(s["walked"].sum()), int((dead & s["walked"]).sum())
    print(f"{tag}: walked candidate-quadrants {n_walked}, marked among them {n_dead} ({100.0 * n_dead / max(n_walked, 1):.1f} %), "
          f"marked in all {int(dead.sum())}, must-mark {int(s['must_mark'].sum())}")
    if not marking:
        assert not dead.any(), "a narrow walker marked an entry"
        return s
    assert not (dead & ~reach).any(), "a mark without its reach bit"
    assert not (dead & s["must_not"]).any(), f"{int((dead & s['must_not']).sum())} contributors are marked dead"
    missing = s["must_mark"] & ~dead
    assert not missing.any(), f"{int(missing.sum())} of {int(s['must_mark'].sum())} must-mark entries are unmarked"
    return s


def _check_single(name, C, compact=False):
    sc, f, b = _case(name, C)
    W, H = SCENES[name]["W"], SCENES[name]["H"]
    marking = C > 4
    _native.set_deterministic(True)
    off, on = _run(sc, False, compact), _run(sc, True, compact)
    _native.set_deterministic(False)
    R = on.num_rendered
    for r in (off, on):
        _check_forward(r, f, sc)
        _check_backward(r, b)          # (the deterministic mode meets the bars of the normal one)
    reach, dead = _full_stream(on.payload, on.state["ranges"], R, compact)
    s = _check_marks(reach, dead, f, W, H, marking, f"{name} C={C}")
    # the switch changes the backward alone
    for k in ("ids", "imask", "idead") + (("cranges", "n_contrib_c", "back") if compact else ()):
        assert torch.equal(off.payload[k], on.payload[k]), k
    for k in ("point_list", "tile_list", "ranges", "n_contrib"):
        assert torch.equal(off.state[k], on.state[k]), k
    assert torch.equal(_bits(off.state["final_T"]), _bits(on.state["final_T"])), "final_T bits"
    for k in ("color", "depth", "alpha"):
        assert torch.equal(_bits(getattr(off, k)), _bits(getattr(on, k))), k + " bits"
    for n in GRADS:
        assert torch.equal(getattr(off, n).grad, getattr(on, n).grad), n
    # float atomics, marks honoured: the oracle bars
    _check_backward(_run(sc, True, compact), b)
    return s, dead


@pytest.mark.parametrize("C", [35, 36, 3])
def test_occluder_scene(C):
    """(a), (c): the wide forward and backward, the chunked C = 36 (its first pass marks) and a narrow layout (unmarked)"""
    s, dead = _check_single("occluder", C)
    if C > 4:
        # the scene does its job on the GPU too: marks in every chunk of the long list, and more of them than the pixel-missing
        # Gaussians alone (occluded footprints)
        in_list = s["tile"] == 0
        chunk = s["pos"] // 64
        for c in range(3):
            assert (dead & s["walked"])[in_list & (chunk == c)].any(), f"no walked entry of chunk {c} is marked"
        assert int((dead & s["walked"]).sum()) > int(s["must_mark"].sum())
        assert int((dead & s["walked"]).sum()) >= 0.05 * int(s["walked"].sum())


@pytest.mark.parametrize("name", ["edge", "edge_row"])
def test_quadrants_outside_the_image(name):
    """(d): 40 x 24 — the scene's tile has two quadrants without a pixel"""
    _check_single(name, 35)


def test_compact_stream_behind_the_radix_front_end():
    """the headline's own stream: live entries only, the backward bounded by n_contrib_c — marks sit on compact positions"""
    _native.set_front_end(0)
    _check_single("occluder", 35, compact=True)


def _frame_payload(f, W, H):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in introspect.payload_state((f.geom, f.binning, f.img), sum(f.R), W, H, V=f.V, compact=False).items()}


def test_second_forward_over_the_same_buffers_leaves_the_same_marks():
    import ctypes as C
    from splatloc_amd import rasterizer as rz
    sc, _, _ = _case("occluder", 35)
    dev = torch.device(DEV)
    from tests.test_gpu_window import _views
    views = _views(sc, 2, dev)
    t = lambda x: x.to(dev).contiguous()  # noqa: E731
    f = rz.window_forward(t(sc.means3D), t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations), None, [rs for _, rs, _ in views])
    W, H = sc.camera.image_width, sc.camera.image_height
    first = _frame_payload(f, W, H)
    assert int(first["idead"].count_nonzero()) > 0
    images = [x.clone() for x in (f.color, f.depth, f.alpha)]
    # the same launch sequence once more into the SAME geometry / binning / image buffers
    lib = _native.load()
    wv = rz._window_views(f)
    R = (C.c_int64 * f.V)()
    with rz._on_device(dev):
        _native.check(lib.splatraster_forward_window_geometry(
            C.byref(f.st), f.V, wv, f.P, rz._ptr(f.m3), rz._ptr(f.opa), rz._ptr(f.sca), rz._ptr(f.rot), rz._ptr(f.cov), rz._ptr(f.geom), R,
            rz._stream(dev)), "forward_window_geometry")
        assert [int(r) for r in R] == f.R
        _native.check(lib.splatraster_forward_window_render(
            C.byref(f.st), f.V, wv, f.P, R, rz._ptr(f.bg), rz._ptr(f.col), rz._ptr(f.geom), rz._ptr(f.binning), rz._ptr(f.img),
            rz._stream(dev)), "forward_window_render")
    second = _frame_payload(f, W, H)
    for k in ("ids", "imask", "idead"):
        assert torch.equal(first[k], second[k]), k
    for a, b in zip(images, (f.color, f.depth, f.alpha)):
        assert torch.equal(_bits(a), _bits(b))


def test_window_of_two_views_with_different_cameras():
    """(b): V = 2, the second view's rows start at row0 = P; marks per view against that view's own oracle forward, summed
    gradients torch.equal between on and off in the deterministic mode and at the oracle's bars in the normal one"""
    from oracle import oracle
    from splatloc_amd import rasterize_window
    from tests.test_gpu_window import NAMES, _leaves, _views
    sc, _, _ = _case("occluder", 35)
    P, V = sc.means3D.shape[0], 2
    W, H = sc.camera.image_width, sc.camera.image_height
    dev = torch.device(DEV)
    views = _views(sc, V, dev)
    fs, tot, m2o = [], {}, []
    for cam, rs, g in views:
        f = oracle.forward(oracle.Settings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy), sc.bg.numpy(),
                           sc.means3D.numpy(), sc.opacities.numpy(), cam.world_view_transform.cpu().numpy(),
                           cam.full_proj_transform.cpu().numpy(), cam.camera_center.cpu().numpy(),
                           colors_precomp=sc.features.numpy(), scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), omp=True)
        b = oracle.backward(f, g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy(), omp=True)
        for k, _ in NAMES:
            tot[k] = b[k].astype(np.float64) + tot.get(k, 0.0)
        m2o.append(b["dL_dmeans2D"])
        fs.append(f)

    def run(marks, det):
        _native.set_dead_marks(marks)
        _native.set_deterministic(det)
        L = _leaves(sc, dev)
        m2s = [torch.zeros_like(L["means3D"], requires_grad=True) for _ in views]
        outs = rasterize_window([rs for _, rs, _ in views], L["means3D"], m2s, L["colors"], L["opac"], scales=L["scales"], rotations=L["rots"])
        fn = outs[0][0].grad_fn
        bufs = introspect.forward_buffers(fn)
        st = [{k: v.clone() for k, v in d.items()} for d in introspect.window_state(bufs, P, V, W, H, fn.R)]
        pay = {k: v.clone() for k, v in introspect.payload_state(bufs, sum(fn.R), W, H, V=V, compact=False).items()}
        loss = 0
        for (color, depth, alpha, _), (_, _, g) in zip(outs, views):
            loss = loss + (color * g[0]).sum() + (depth * g[1]).sum() + (alpha * g[2]).sum()
        loss.backward()
        torch.cuda.synchronize()
        _native.set_deterministic(False)
        return L, outs, m2s, st, pay, list(fn.R)

    L0, o0, m0, s0, p0, R0 = run(False, True)
    L1, o1, m1, s1, p1, R1 = run(True, True)
    assert R0 == R1 == [int(f["num_rendered"]) for f in fs] and min(R0) > 0
    reach, dead = _quads(p1["imask"]), _quads(p1["idead"])
    at = 0
    for v, f in enumerate(fs):       # the window's stream: view 0's lists, then view 1's; ids are rows v * P + i
        sl = slice(at, at + R1[v])
        assert np.array_equal(p1["ids"][sl].cpu().numpy().astype(np.int64), f["point_list"].astype(np.int64) + v * P), v
        _check_marks(reach[sl], dead[sl], f, W, H, True, f"window view {v}")
        assert dead[sl].any()
        at += R1[v]
    for k in ("ids", "imask", "idead"):
        assert torch.equal(p0[k], p1[k]), k
    for v in range(V):
        for k in ("point_list", "tile_list", "ranges", "n_contrib"):
            assert torch.equal(s0[v][k], s1[v][k]), (v, k)
        assert torch.equal(_bits(s0[v]["final_T"]), _bits(s1[v]["final_T"]))
        for i in range(3):
            assert torch.equal(_bits(o0[v][i]), _bits(o1[v][i])), (v, i)
        assert torch.equal(m0[v].grad, m1[v].grad)
    for _, nm in NAMES:
        assert torch.equal(L0[nm].grad, L1[nm].grad), nm
    L2, _, m2, _, _, _ = run(True, False)
    for v in range(V):
        assert_grad_close(f"means2D[{v}]", m2[v].grad.cpu().numpy(), m2o[v])
    for k, nm in NAMES:
        assert_grad_close(k, L2[nm].grad.cpu().numpy(), tot[k])


def _ipack_words(run, sc):
    """the payload words of a run's forward, as a VIEW into its binning buffer (full stream)"""
    cam = sc.camera
    _geom, binning, _img = introspect.forward_buffers(run.color.grad_fn)
    sp = introspect.binning_spans(1, run.num_rendered, cam.image_width, cam.image_height)
    # (.data: the buffer is saved for the backward, and this write is meant to reach it without autograd's version check)
    return introspect._view(binning.data, sp["ipack"], int(run.num_rendered), torch.int32)


@pytest.mark.parametrize("marks", [True, False])
def test_backward_skips_exactly_what_is_marked(marks):
    """The only test in which the backward's skipping is observable: every entry of the stream is marked dead for every quadrant by
    hand between the forward and the backward.  With the marks honoured the backward then walks nothing — every gradient is zero;
    with the switch off it ignores them and the gradients meet the oracle's bars."""
    sc, f, b = _case("occluder", 35)
    _native.set_dead_marks(marks)
    r = HipRun(sc, backward=False)
    words = _ipack_words(r, sc)
    words |= -268435456          # 0xF0000000 as int32: bits 28..31
    dev = r.color.device
    ((r.color * sc.dL_dcolor.to(dev)).sum() + (r.depth * sc.dL_ddepth.to(dev)).sum() + (r.alpha * sc.dL_dalpha.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    if marks:
        for n in GRADS:
            assert int(getattr(r, n).grad.count_nonzero()) == 0, n
    else:
        _check_backward(r, b)


def _spy_frames(monkeypatch):
    """the frames the autograd adapters render into (under no_grad the outputs carry no grad_fn to reach the buffers through)"""
    from splatloc_amd import rasterizer as rz
    frames = []

    def spy(fn):
        def wrapped(*a, **k):
            f = fn(*a, **k)
            frames.append((f, bool(k.get("forward_only", False))))
            return f
        return wrapped
    monkeypatch.setattr(rz, "view_forward", spy(rz.view_forward))
    monkeypatch.setattr(rz, "window_forward", spy(rz.window_forward))
    return frames


@pytest.mark.parametrize("leaves", ["parameters_under_no_grad", "plain_tensors"])
def test_forward_only_render_writes_no_marks(leaves, monkeypatch):
    """No backward can follow — trained parameters (requires_grad = True leaves) rendered under torch.no_grad(), as the evaluation
    renders do, or inputs none of which wants a gradient: the render is told so and leaves bits 28..31 alone, through
    GaussianRasterizer and through rasterize_window; its images are those of the marking render, bit for bit.  The same leaves
    with grad mode on are marked (every other test of this file)."""
    from splatloc_amd import GaussianRasterizer, rasterize_window
    from tests.helpers import hip_settings
    sc, f, _ = _case("occluder", 35)
    dev = torch.device(DEV)
    cam = sc.camera
    W, H = cam.image_width, cam.image_height
    ref = _run(sc, True, backward=False)
    assert int(ref.payload["idead"].count_nonzero()) > 0
    frames = _spy_frames(monkeypatch)
    want = leaves == "parameters_under_no_grad"
    t = lambda x: torch.nn.Parameter(x.to(dev).contiguous()) if want else x.to(dev).contiguous()  # noqa: E731
    m3, col, opa, sca, rot = t(sc.means3D), t(sc.features), t(sc.opacities), t(sc.scales), t(sc.rotations)
    carrier = lambda: torch.zeros_like(m3).requires_grad_(want)  # noqa: E731
    rs = hip_settings(sc, dev)
    import contextlib
    with (torch.no_grad() if want else contextlib.nullcontext()):
        color, depth, alpha, radii = GaussianRasterizer(raster_settings=rs)(
            means3D=m3, means2D=carrier(), shs=None, colors_precomp=col, opacities=opa, scales=sca, rotations=rot, cov3D_precomp=None)
        wouts = rasterize_window([rs, rs], m3, [carrier(), carrier()], col, opa, scales=sca, rotations=rot)
    torch.cuda.synchronize()
    assert color.grad_fn is None and wouts[0][0].grad_fn is None
    assert len(frames) == 2 and all(flag for _, flag in frames), "the adapters did not say that no backward follows"
    fv, fw = frames[0][0], frames[1][0]
    pv = introspect.payload_state((fv.geom, fv.binning, fv.img), fv.num_rendered, W, H, compact=False)
    pw = introspect.payload_state((fw.geom, fw.binning, fw.img), sum(fw.R), W, H, V=2, compact=False)
    assert int(pv["idead"].count_nonzero()) == 0 and int(pw["idead"].count_nonzero()) == 0
    assert torch.equal(pv["imask"], ref.payload["imask"]) and torch.equal(pv["ids"], ref.payload["ids"])
    for a, bb in ((color, ref.color), (depth, ref.depth), (alpha, ref.alpha)):
        assert torch.equal(_bits(a), _bits(bb.detach()))
    for v in range(2):
        for a, bb in zip(wouts[v][:3], (ref.color, ref.depth, ref.alpha)):
            assert torch.equal(_bits(a), _bits(bb.detach()))


def test_render_with_grad_mode_on_is_told_that_a_backward_follows(monkeypatch):
    """the other side of the decision: leaves that want a gradient, grad mode on"""
    sc, _, _ = _case("occluder", 35)
    frames = _spy_frames(monkeypatch)
    HipRun(sc, backward=False)
    assert len(frames) == 1 and not frames[0][1]
