"""Landmark selection on the MI355X at the edges of its kernels (csrc/selection.hip): every launch-shape boundary of the score
kernel, its strict thresholds, the Jacobi solver and the one-pass statistics at their degenerate inputs, depth offsets beyond
2^31, the score key and both sort passes at special values and at every path of the sort and the scan, the resolve kernel's
chunk loop and its landmarks beyond the LDS batch, the filter's batches and early exit, the distance rounding, and the
workspace of the C ABI.  The references, the bars and the proof that every case reaches its edge are in
tests/selection_reference.py and tests/test_host_selection_edges.py; nothing here is compared with a device result."""
import ctypes as C

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import selection as S
from splatloc_amd.rasterizer import _stream
from tests import selection_reference as R
from tests.test_host_selection import greedy_pick, priority_order, scores_f64

pytestmark = pytest.mark.gpu


def _device_scores(s):
    out = S.landmark_scores(s["points"], s["w2cs"], s["K"], s["depths"], width=s["width"], height=s["height"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_scores(s, what, window=None):
    """device against the exact counts of the restatement and the bars of tests/selection_reference.py"""
    win = s if window is None else dict(s, depths=window)
    ref = R.reference_and_bars(win["points"], win["w2cs"], win["K"], win["depths"], win["width"], win["height"])
    got = _device_scores(s)
    if len(s["w2cs"]):
        rest = scores_f64(win["points"], win["w2cs"], win["K"], win["depths"], win["width"], win["height"])
        assert np.array_equal(got["n_visible"], rest["n_visible"]) and np.array_equal(got["n_depth"], rest["n_depth"]), what
    worst = R.check_device_scores(got, ref, what)
    print(f"{what}: worst err / bar {worst}")
    return got, ref


# ---- A. scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.GRID_M)
def test_scores_launch_shape_grid(M):
    for N in R.GRID_N:
        got, ref = _check_scores(R.grid_case(N, M), f"grid N={N} M={M}")
        if M == 0:
            assert not got["n_visible"].any() and not got["n_depth"].any() and np.all(got["span"] == 0.0)
            assert np.isnan(got["depth_mean"]).all() and np.isnan(got["depth_std"]).all() and np.all(got["score"] == 4.0)


def test_scores_strict_thresholds():
    scene, rows = R.threshold_case()
    got, _ = _check_scores(scene, "thresholds")
    for i, (name, nv, nd, mean) in enumerate(rows):
        assert (got["n_visible"][i], got["n_depth"][i]) == (nv, nd), name
        if mean is None:
            assert np.isnan(got["depth_mean"][i]), name
        else:
            assert got["depth_mean"][i] == mean and got["depth_std"][i] == 0.0, name     # the pixel that was gathered
    _check_scores(R.permuted_threshold_case(), "permuted poses")


@pytest.mark.parametrize("K", [R.GENERAL_K, R.ZERO_ROW_K], ids=["skew and third row", "q2 == 0"])
def test_scores_general_intrinsics(K):
    _check_scores(R.general_k_case(K), f"K third row {K[2]}")


@pytest.mark.parametrize("width,height", R.IMAGE_SHAPES)
def test_scores_image_shapes(width, height):
    _check_scores(R.image_case(width, height), f"{width} x {height}")


def test_scores_crop_of_a_larger_stack():
    s = R.crop_case()
    assert s["depths"].shape[1:] == (47, 53)
    _check_scores(s, "crop", window=np.ascontiguousarray(s["depths"][:, :30, :40]))
    # the same through a device tensor, which selection.py crops on the device
    dev = dict(s, depths=torch.from_numpy(s["depths"]).cuda())
    got = _device_scores(dev)
    ref = scores_f64(s["points"], s["w2cs"], s["K"], s["depths"][:, :30, :40], 40, 30)
    assert np.array_equal(got["n_depth"], ref["n_depth"]) and np.array_equal(got["n_visible"], ref["n_visible"])


def test_scores_jacobi_edges():
    if not R.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa here: no span bars")
    for name, s in R.jacobi_cases().items():
        got, ref = _check_scores(s, f"jacobi {name}")
        if name == "isotropic":
            assert got["span"][0] == np.pi / 2
        if name == "rank-1 complement":
            assert got["n_visible"][0] >= 2 and abs(np.cos(got["span"][0]) - 1.0) <= R.SPAN_C_BAR


def test_scores_statistics_edges():
    for name, (s, prop) in R.statistics_cases().items():
        got, ref = _check_scores(s, f"statistics {name}")
        if prop == "equal":
            d = ref["mean"][0]
            assert got["depth_std"][0] == 0.0 and got["depth_mean"][0] == d
            assert got["score"][0] == 0.05 / d + 2.0 + got["span"][0]                   # the std half saturates at 2
        else:
            assert got["n_depth"][0] == prop


def test_scores_depth_offsets_beyond_2_31():
    M, H, W = R.BIG["M"], R.BIG["H"], R.BIG["W"]
    need = M * H * W * 4
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * need:
        pytest.skip(f"{free} bytes free, the test needs 1.5 x {need}")
    pts, w2cs, K, marks = R.big_case()
    stack = torch.full((M, H, W), R.BIG["fill"], dtype=torch.float32, device="cuda")
    for (v, r, c), d in marks.items():
        stack[v, r, c] = float(d)
    try:
        out = S.landmark_scores(pts, w2cs, K, stack, width=W, height=H)
        got = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        del stack
        torch.cuda.empty_cache()
    rest = R.scores_f64_lookup(pts, w2cs, K, R.big_lookup(marks), W, H)
    assert np.array_equal(got["n_visible"], rest["n_visible"]) and np.array_equal(got["n_depth"], rest["n_depth"])
    ref = R.reference_and_bars(pts, w2cs, K, R.LookupStack(R.big_lookup(marks)), W, H)
    print("big stack: worst err / bar", R.check_device_scores(got, ref, "big stack"))


# ---- B. order -------------------------------------------------------------------------------------------------------------------
def _select(points, scores, num, radius):
    idx, passes = S.select_landmarks(torch.from_numpy(points).cuda(), torch.from_numpy(scores).cuda(), num, radius,
                                     return_passes=True)
    return idx.cpu().numpy(), passes


def test_order_of_special_scores():
    pts = R.lattice_points(3000)
    for scores in (R.special_scores(3000), np.full(3000, 1.25), np.full(3000, np.nan)):
        idx, passes = _select(pts, scores, 3000, 0.25)
        assert np.array_equal(idx, priority_order(scores)) and passes == 1
    assert np.array_equal(idx, np.arange(3000)[::-1])


@pytest.mark.parametrize("N", R.SORT_SIZES)
def test_order_through_every_sort_and_scan_path(N):
    pts, scores = R.lattice_points(N), R.tied_scores(N)
    idx, passes = _select(pts, scores, 3000, 0.25)
    assert np.array_equal(idx, priority_order(scores)[:3000]) and passes == 1


# ---- C. pick --------------------------------------------------------------------------------------------------------------------
def _check_pick(name):
    """device == greedy_pick == the trace, n_passes == len(trace), and a second run is bit-identical"""
    c, want, trace = R.traced(name)
    idx, passes = _select(c["points"], c["scores"], c["num"], c["radius"])
    assert np.array_equal(idx, want), name
    assert passes == len(trace), (name, passes, len(trace))
    assert np.array_equal(want, greedy_pick(c["points"], c["scores"], c["num"], c["radius"])), name
    again, passes2 = _select(c["points"], c["scores"], c["num"], c["radius"])
    assert np.array_equal(again, idx) and passes2 == passes, name
    return c, idx, trace


@pytest.mark.parametrize("num", [5000, 4096, 4097, 4098])
def test_pick_more_landmarks_in_a_pass_than_the_lds_batch(num):
    _check_pick(f"many landmarks, num {num}")


@pytest.mark.parametrize("S_", R.CHUNK_SURVIVORS)
@pytest.mark.parametrize("kind", ["far", "near"])
def test_pick_chunk_boundaries(kind, S_):
    _check_pick(f"chunk {kind} {S_}")


def test_pick_num_reached_inside_and_at_the_start_of_a_chunk():
    _check_pick("num at first of chunk 2")
    _check_pick("num inside chunk 1")


@pytest.mark.parametrize("L", R.FILTER_COUNTS)
def test_pick_filter_boundaries(L):
    _check_pick(f"filter {L}")


def test_pick_exact_lattice():
    c, idx, trace = _check_pick("lattice at r")
    assert len(trace) == 1                                          # < is strict: spacing r, all taken at once
    c, idx, trace = _check_pick("lattice under r")
    assert len(trace) > 1


@pytest.mark.parametrize("i", range(3))
def test_pick_rounding_sensitive_pair(i):
    c, idx, trace = _check_pick(f"rounding pair {i}")
    assert list(idx) == [0, 3, 4, 1]


def test_pick_duplicates_and_signed_zeros():
    dup = R.duplicates_case()
    c, idx, trace = _check_pick("duplicates")
    assert not set(idx) & set(dup["losers"])
    with pytest.raises(ValueError, match="distinct"):
        S.select_landmarks(dup["points"], dup["scores"], dup["distinct"] + 1, dup["radius"])


def test_pick_long_pass_count():
    c, idx, trace = _check_pick("long pass count")
    assert any(t["survivors"] == 0 for t in trace) and len(trace) >= 95


# ---- D. ABI ---------------------------------------------------------------------------------------------------------------------
GUARD = 4096
PATTERN = 0xA5


def _abi_select(c, buf=None, fill=None, extra=0):
    """splatraster_landmark_select with the workspace inside a patterned buffer, GUARD bytes of it on either side, and out_idx
    followed by 1024 patterned entries.  Returns out_idx[:num], n_passes, the buffer, and whether every guard is intact."""
    lib = _native.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.from_numpy(np.ascontiguousarray(c["points"], np.float32)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(c["scores"], np.float64)).to(dev)
    N, num = len(c["points"]), int(c["num"])
    nbytes = int(lib.splatraster_landmark_workspace_bytes(N, num))
    if buf is None:
        buf = torch.full((GUARD + nbytes + extra + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.numel() >= GUARD + nbytes + GUARD and (buf.data_ptr() + GUARD) % 256 == 0
    if fill is not None:
        buf[GUARD:GUARD + nbytes] = fill
    out = torch.full((num + 1024,), -1, dtype=torch.int32, device=dev)
    out.view(torch.uint8)[:] = PATTERN
    passes = C.c_int32(-1)
    st = lib.splatraster_landmark_select(N, C.c_void_p(p.data_ptr()), C.c_void_p(s.data_ptr()), num, float(c["radius"]),
                                         C.c_void_p(out.data_ptr()), C.byref(passes), C.c_void_p(buf.data_ptr() + GUARD),
                                         _stream(dev))
    torch.cuda.synchronize()
    assert st == 0, st
    intact = bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + nbytes:] == PATTERN).all()) \
        and bool((out[num:].view(torch.uint8) == PATTERN).all())
    return out[:num].cpu().numpy(), int(passes.value), buf, intact


def _tiny_case(N, num):
    rng = np.random.default_rng(N + num)
    return dict(points=R.lattice_points(N)[rng.permutation(N)], scores=rng.integers(0, 5, N).astype(np.float64), num=num,
                radius=1.5)


@pytest.mark.parametrize("name", ["N=1 num=1", "N=257 num=257", "N=4097 num=1", "filter 257", "chunk near 1025"])
def test_abi_workspace_guards(name):
    c = {"N=1 num=1": lambda: _tiny_case(1, 1), "N=257 num=257": lambda: _tiny_case(257, 257),
         "N=4097 num=1": lambda: _tiny_case(4097, 1)}.get(name, lambda: R.traced(name)[0])()
    idx, passes, _, intact = _abi_select(c)
    assert intact, name
    want, trace = R.greedy_trace(c["points"], c["scores"], c["num"], c["radius"])
    assert np.array_equal(idx, want) and passes == len(trace)


def test_abi_workspace_state_does_not_matter():
    c, want, trace = R.traced("filter 513")
    other = R.traced("chunk far 2049")[0]
    lib = _native.load()
    extra = max(0, int(lib.splatraster_landmark_workspace_bytes(len(other["points"]), other["num"]))
                - int(lib.splatraster_landmark_workspace_bytes(len(c["points"]), c["num"])))
    results = []
    for fill in (0x00, 0xFF):
        idx, passes, buf, _ = _abi_select(c, fill=fill, extra=extra)
        results.append((idx, passes))
    _abi_select(other, buf=buf)                                  # leaves its own state behind
    idx, passes, _, _ = _abi_select(c, buf=buf)
    results.append((idx, passes))
    for idx, passes in results:
        assert np.array_equal(idx, want) and passes == len(trace)
