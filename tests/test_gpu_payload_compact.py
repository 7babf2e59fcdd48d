"""The payload compacted to the live instances (csrc/binning.hip: payload_tile_kernel) against the full stream of payload_kernel
and against the CPU oracle — needs an MI355X.

Behind the radix front end the compositing kernels stream, per (view, tile) list, only the instances whose reach mask is not 0.
That changes the stream (irec / ipack, the table cranges, the plane n_contrib_c) and nothing else: radii, num_rendered,
point_list, tile_list, ranges, n_contrib and final_T are the oracle's, bit for bit, with compaction on and off; colours, depth and
alpha are bit-identical between the two for C <= 4 and C = 32..35 (a list-ordered fmaf chain whatever the pairing) and meet the
oracle bar at C = 40 (pair sums: which candidates share a pair changes the last bit); gradients are torch.equal in the
deterministic mode and meet the existing bars otherwise.

Scenes are small but hold real dead instances (every test asserts >= 20 % of them with compaction off); the directed lists put
known numbers of live and dead entries into single tiles: a Gaussian 0.002 wide projects to sigma^2 ~ 0.3 px^2 (the dilation) and
a 3 px radius, so one centred >= 3 px inside a tile touches that tile alone, and one centred 1.4 px right of a tile border with
opacity 0.02 touches the tile on the left as well but reaches none of its pixel centres (q = 2.4^2 / 0.31 = 18.6 against
2 ln(255 x 0.02) = 3.3): dead there, live at home.  Narrow layouts of small frames are split launches by default, which keep the
full stream; the tests switch the split off (on both sides) so that the one-wave narrow kernel walks the compact stream.
"""
import pytest
import torch

from splatloc_amd import _native, introspect
from splatloc_amd.synthetic import make_scene
from tests.helpers import HipRun, oracle_backward, oracle_forward
from tests.test_gpu_parity import _check_backward, _check_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("means3D", "means2D", "opacities", "colors", "scales", "rotations")


@pytest.fixture(autouse=True)
def _radix_front_end_whole_lists():
    lib = _native.load()
    _native.set_front_end(0)
    _native.check(lib.splatraster_debug_set_split_max_waves(0), "split_max_waves")
    yield
    _native.set_front_end(-1)
    _native.set_payload_compact(-1)
    _native.set_deterministic(False)
    _native.check(lib.splatraster_debug_set_split_max_waves(-1), "split_max_waves")
    _native.check(lib.splatraster_debug_set_payload_stream_min(-1), "payload_stream_min")


def _run(sc, compact, backward=True):
    """HipRun with the stream the compositing kernels read attached (`payload`, copied before the backward frees the buffers)"""
    _native.set_payload_compact(-1 if compact else 0)
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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_stream(off, on, min_dead=0.2):
    """the compact stream = the live entries of the full one, list by list, in order; what the forward derives from it"""
    imask = off.payload["imask"]
    live = imask != 0
    R = off.num_rendered
    assert R == on.num_rendered and imask.numel() == R
    dead = 1.0 - float(live.float().mean())
    assert dead >= min_dead, f"only {dead:.3f} of the instances are dead: the scene does not test the compaction"
    for k in ("tiles_touched", "point_list", "tile_list", "ranges", "n_contrib"):
        assert torch.equal(off.state[k], on.state[k]), k
    assert torch.equal(_bits(off.state["final_T"]), _bits(on.state["final_T"])), "final_T bits"
    assert torch.equal(off.radii, on.radii)
    # the full stream is payload_kernel's: ids = point_list, in order
    assert torch.equal(off.payload["ids"], off.state["point_list"])
    tl, rng = off.state["tile_list"].long(), off.state["ranges"].long()
    cr = on.payload["cranges"].long()
    lens = torch.bincount(tl[live], minlength=rng.shape[0])
    assert torch.equal(cr[:, 0], rng[:, 0]), "a compact list starts where its list starts"
    assert torch.equal(cr[:, 1] - cr[:, 0], lens), "live entries per list"
    assert int(lens.sum()) == on.payload["ids"].numel() < R        # the compaction was in effect
    assert torch.equal(on.payload["ids"], off.payload["ids"][live]) and torch.equal(on.payload["imask"], imask[live])
    keep = [0, 1, 2, 4, 5, 6, 7]    # (column 3: the radius in the full stream, the way back to the list position in the compact one)
    assert torch.equal(_bits(on.payload["irec"][:, keep]), _bits(off.payload["irec"][live][:, keep]))
    pos = torch.arange(R, device=tl.device) - rng[tl, 0] + 1
    assert torch.equal(on.payload["back"].long(), pos[live]), "the moved word: list position + 1"
    # n_contrib_c: the rank, among the live entries of the pixel's tile, of the entry n_contrib names
    nc, ncc = on.state["n_contrib"].long(), on.payload["n_contrib_c"][0].long()
    H, W = nc.shape
    gx = (W + 15) // 16
    tile_of_pixel = (torch.arange(H, device=nc.device)[:, None] // 16) * gx + torch.arange(W, device=nc.device)[None, :] // 16
    assert torch.equal(ncc == 0, nc == 0)
    hit = nc > 0
    j = rng[tile_of_pixel[hit], 0] + nc[hit] - 1                   # instance index of the pixel's last contributor
    assert bool(live[j].all()), "a last contributor is a live instance"
    rank = torch.cumsum(live.long(), 0)                            # live entries up to and including j, over the whole stream
    before = torch.zeros_like(rank)
    before[1:] = rank[:-1]
    assert torch.equal(ncc[hit], rank[j] - before[rng[tile_of_pixel[hit], 0]])
    return lens


def _check_pair(sc, C, min_dead=0.2, images_bit_identical=True, gradients_bit_identical=True):
    """compaction on against off and both against the oracle; returns (off, on, live entries per list)"""
    f = oracle_forward(sc)
    b = oracle_backward(f, sc)
    _native.set_deterministic(True)
    off, on = _run(sc, False), _run(sc, True)
    _native.set_deterministic(False)
    lens = _check_stream(off, on, min_dead)
    for r in (off, on):
        _check_forward(r, f, sc)
        _check_backward(r, b)
    if images_bit_identical:
        for k in ("color", "depth", "alpha"):
            assert torch.equal(_bits(getattr(off, k)), _bits(getattr(on, k))), k + " bits"
    if gradients_bit_identical:
        for n in GRADS:
            assert torch.equal(getattr(off, n).grad, getattr(on, n).grad), n
    _check_backward(_run(sc, True), b)      # float atomics: the existing bars
    return off, on, lens


@pytest.mark.parametrize("C,seed", [(3, 31), (4, 32), (35, 33)])
def test_ragged_frame_on_equals_off_equals_oracle(C, seed):
    _check_pair(make_scene(3000, 333, 201, C, seed, scale_median=0.03), C)


def test_chunked_wide_layout_meets_the_oracle_bar():
    """C = 40 = 32 + 8: pair sums (acc += f0 w0 + f1 w1) round by who shares a pair — the oracle bar, not bit identity"""
    _check_pair(make_scene(1500, 160, 96, 40, 25, scale_median=0.04), 40, images_bit_identical=False, gradients_bit_identical=False)


# ---- directed lists ---------------------------------------------------------------------------------------------------------------
# (live entries, dead entries, their order in depth, opacity of the live ones): slot k is tile (2 (k % 4), k // 4) of a 125 x 30
# frame, its dead entries live in the tile to its right.  Opacity 0.03: 257 entries leave T = 4e-4 > 1e-4, so every live entry
# contributes and the centre pixel's last contributor is the list's last live entry; 0.6: the centre pixel is finished after ten
# entries, its neighbours after seventy, the pixels two away never — last contributors all over the list, dead runs on both sides.
SLOTS = [(63, 192, "mixed", 0.03), (64, 192, "dead_first", 0.03), (65, 192, "live_first", 0.03), (255, 258, "mixed", 0.03),
         (256, 1, "mixed", 0.03), (257, 0, "mixed", 0.03), (0, 100, "mixed", 0.03), (300, 300, "mixed", 0.6)]


def _place(sc, s, px, py, z, opacity):
    cam = sc.camera
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    sc.means3D[s, 0] = (px - (W - 1) / 2.0) / fx * z
    sc.means3D[s, 1] = (py - (H - 1) / 2.0) / fy * z
    sc.means3D[s, 2] = z
    sc.scales[s] = 0.002
    sc.opacities[s, 0] = opacity


def _directed_scene(C, seed=5):
    n = sum(a + b for a, b, _, _ in SLOTS)
    sc = make_scene(n, 125, 30, C, seed, scale_median=0.02)
    g = torch.Generator().manual_seed(seed)
    at = 0
    for k, (nl, nd, pattern, op) in enumerate(SLOTS):
        tx, ty, m = 2 * (k % 4), k // 4, nl + nd
        is_live = torch.arange(m) < nl
        order = {"mixed": torch.randperm(m, generator=g), "dead_first": torch.cat([torch.arange(nl, m), torch.arange(nl)]),
                 "live_first": torch.arange(m)}[pattern]          # order[r]: the member at depth rank r
        z = torch.empty(m)
        z[order] = 1.0 + 3.0 * (torch.arange(m, dtype=torch.float32) + 0.5) / m
        px = torch.where(is_live, torch.tensor(16.0 * tx + 5.3), torch.tensor(16.0 * (tx + 1) + 1.4))
        _place(sc, slice(at, at + m), px, torch.full((m,), 16.0 * ty + 6.6), z, torch.where(is_live, torch.tensor(op), torch.tensor(0.02)))
        at += m
    return sc


@pytest.mark.parametrize("C", [3, 35])
def test_directed_lists(C):
    sc = _directed_scene(C)
    off, on, live = _check_pair(sc, C)
    rng = off.state["ranges"].long()
    full = rng[:, 1] - rng[:, 0]
    imask, tl = off.payload["imask"], off.state["tile_list"].long()
    nc = on.state["n_contrib"]
    for k, (nl, nd, pattern, _) in enumerate(SLOTS):
        t = (k // 4) * 8 + 2 * (k % 4)
        assert (int(full[t]), int(live[t])) == (nl + nd, nl), (k, int(full[t]), int(live[t]))
        m = imask[tl == t]
        tile_nc = nc[16 * (k // 4):16 * (k // 4) + 16, 32 * (k % 4):32 * (k % 4) + 16]
        if nl == 0:     # touched by dead instances only: nothing to stream, nobody contributes
            assert int(tile_nc.max()) == 0
            continue
        if pattern == "dead_first":
            assert int(m[0]) == 0 and int(m[-1]) != 0          # a live entry last in its list, behind a dead run
        if pattern == "live_first":
            assert int(m[0]) != 0 and int(m[-1]) == 0          # a live entry first in its list, a dead run behind the last contributor
            assert int(tile_nc.max()) == nl
        if pattern == "dead_first":
            assert int(tile_nc.max()) == nl + nd
    # slot 7: last contributors in the middle of the list, dead entries in front of and behind them
    last = nc[16:30, 96:112]
    mid = last[(last > 0) & (last < 600)]
    assert mid.numel() > 0 and int(mid.min()) < 100
    assert {(63, 255), (64, 256), (65, 257), (255, 513), (256, 257), (257, 257)} <= {(int(a), int(b)) for a, b in zip(live, full)}


def _long_list_scene(C, n_live, n_dead, seed):
    """one tile (1, 1) of a 64 x 48 frame with n_live entries spread over 16 of its pixels, and n_dead from the tile to its right"""
    m = n_live + n_dead
    sc = make_scene(m, 64, 48, C, seed, scale_median=0.02)
    g = torch.Generator().manual_seed(seed)
    z = torch.empty(m)
    z[torch.randperm(m, generator=g)] = 1.0 + 3.0 * (torch.arange(m, dtype=torch.float32) + 0.5) / m
    i = torch.arange(m)
    is_live = i < n_live
    px = torch.where(is_live, 16.0 + 3.3 + 3.0 * (i % 4), torch.tensor(32.0 + 1.4))
    py = 16.0 + 3.3 + 3.0 * ((i // 4) % 4)
    _place(sc, slice(0, m), px, py, z, torch.where(is_live, torch.tensor(0.03), torch.tensor(0.02)))
    return sc


def test_long_list_all_live():
    """9 000 entries, all live in their own tile (the scene's dead instances are what the 3 px rects put into the tiles above and
    to the left: lists of dead entries only)"""
    sc = _long_list_scene(35, 9000, 0, 61)
    off, on, live = _check_pair(sc, 35)
    rng = off.state["ranges"].long()
    assert int(rng[5, 1] - rng[5, 0]) == 9000 == int(live[5]) and int(on.state["n_contrib"].max()) > 4096


def test_long_list_mostly_dead_with_streaming_stores():
    """9 000 entries of which 500 are live; the payload written with the streaming stores of large windows"""
    _native.check(_native.load().splatraster_debug_set_payload_stream_min(0), "payload_stream_min")
    sc = _long_list_scene(4, 500, 8500, 62)
    off, on, live = _check_pair(sc, 4)
    rng = off.state["ranges"].long()
    t = 1 * 4 + 1
    assert int(rng[t, 1] - rng[t, 0]) == 9000 and int(live[t]) == 500


def test_window_with_a_view_that_renders_nothing():
    """Five views in one launch sequence, the third looks away: per-view state and images identical with compaction on and off,
    summed gradients torch.equal in the deterministic mode and at the oracle's bar"""
    from splatloc_amd import rasterize_window
    from tests.test_gpu_accumulator_layout import NAMES, _oracle, _views
    from tests.helpers import assert_grad_close
    from tests.test_gpu_window import _leaves
    sc = make_scene(3000, 333, 201, 35, 34, scale_median=0.03)
    P, V, W, H = 3000, 5, 333, 201
    dev = torch.device(DEV)
    views = _views(sc, V, dev, away=(2,))
    tot, m2o = _oracle(sc, views)
    res = {}
    _native.set_deterministic(True)
    for compact in (False, True):
        _native.set_payload_compact(-1 if compact else 0)
        L = _leaves(sc, dev)
        m2s = [torch.zeros_like(L["means3D"], requires_grad=True) for _ in views]
        outs = rasterize_window([rs for _, rs, _ in views], L["means3D"], m2s, L["colors"], L["opac"], scales=L["scales"], rotations=L["rots"])
        fn = outs[0][0].grad_fn
        bufs = introspect.forward_buffers(fn)
        st = [{k: v.clone() for k, v in d.items()} for d in introspect.window_state(bufs, P, V, W, H, fn.R)]
        pay = {k: v.clone() for k, v in introspect.payload_state(bufs, sum(fn.R), W, H, V=V, compact=compact).items()}
        loss = 0
        for (color, depth, alpha, _), (_, _, g) in zip(outs, views):
            loss = loss + (color * g[0]).sum() + (depth * g[1]).sum() + (alpha * g[2]).sum()
        loss.backward()
        torch.cuda.synchronize()
        res[compact] = (L, outs, m2s, st, pay, list(fn.R))
    _native.set_deterministic(False)
    (L0, o0, m0, s0, p0, R0), (L1, o1, m1, s1, p1, R1) = res[False], res[True]
    assert R0 == R1 and R0[2] == 0 and min(R0[0], R0[1], R0[3], R0[4]) > 0
    live = p0["imask"] != 0
    assert 1.0 - float(live.float().mean()) >= 0.2
    assert p1["ids"].numel() == int(live.sum()) < sum(R0)
    assert torch.equal(p1["ids"], p0["ids"][live]) and torch.equal(p1["imask"], p0["imask"][live])
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    cr = p1["cranges"].view(V, tiles, 2)
    assert int((cr[2, :, 1] - cr[2, :, 0]).abs().max()) == 0 and int(p1["n_contrib_c"][2].max()) == 0
    for v in range(V):
        for k in ("point_list", "tile_list", "ranges", "n_contrib", "tiles_touched"):
            assert torch.equal(s0[v][k], s1[v][k]), (v, k)
        assert torch.equal(_bits(s0[v]["final_T"]), _bits(s1[v]["final_T"]))
        for i in range(3):
            assert torch.equal(_bits(o0[v][i]), _bits(o1[v][i])), (v, i)
        assert torch.equal(o0[v][3], o1[v][3])
        assert torch.equal(m0[v].grad, m1[v].grad)
        assert_grad_close(f"means2D[{v}]", m1[v].grad.cpu().numpy(), m2o[v][0])
    for k, nm in NAMES:
        assert torch.equal(L0[nm].grad, L1[nm].grad), nm
        assert_grad_close(k, L1[nm].grad.cpu().numpy(), tot[k])
