"""csrc/matching.hip at its kernel edges on the MI355X, against the exact host restatements of tests/matching_reference.py
(frustum candidates, descriptor cost) and tests/test_host_matching.py (solver): the inputs the one fixture frame of
tests/test_gpu_matching.py cannot reach.  The host tests pin the restatements to the reference's fixture; here they are the
oracle.  Frustum outputs are compared bit for bit: the file is built without FP contraction, and f64 multiply, add, divide and
square root are correctly rounded on both sides."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import matching as M
from splatloc_amd.rasterizer import _stream
from tests import matching_reference as R
from tests.test_gpu_matching import global_path  # noqa: F401  (fixture)
from tests.test_host_matching import lsap_restated

pytestmark = pytest.mark.gpu


# ---- frustum candidates ---------------------------------------------------------------------------------------------
def _device_frustum(s, key=True):
    out = M.frustum_candidates(s["points"], s["w2c"], s["K"], s["W"], s["H"], **(R.key_args(s) if key else {}))
    return tuple(x.cpu().numpy() for x in out)


def _host_frustum(s, key=True):
    return R.frustum_restated(s["points"], s["w2c"], s["K"], s["W"], s["H"], **(R.key_args(s) if key else {}))


def _assert_bit_equal(got, want, what=""):
    gi, gx, gu = got
    wi, wx, wu = want
    assert gi.dtype == np.int64 and gx.dtype == np.float32 and gu.dtype == np.float64
    assert gi.shape == wi.shape and gx.shape == (len(wi), 3) and gu.shape == (len(wi), 2), (what, gi.shape, wi.shape)
    assert np.array_equal(gi, wi), what
    assert np.array_equal(gx.view(np.int32), wx.view(np.int32)), what
    assert np.array_equal(gu.view(np.int64), np.ascontiguousarray(wu).view(np.int64)), what


def _check_both_modes(s, what=""):
    want = _host_frustum(s)
    _assert_bit_equal(_device_frustum(s), want, what)
    _assert_bit_equal(_device_frustum(s, key=False), _host_frustum(s, key=False), what)
    return want


# N: below the 1 024-bucket floor, at each bucket doubling, several blocks; frames whose pixel count is no multiple of 256;
# mask densities 0, 0.3 and 1
ROOMS = ((1, 1, 1, 1.0), (255, 17, 9, 0.3), (256, 17, 9, 1.0), (257, 64, 48, 0.3), (1023, 64, 48, 1.0),
         (1024, 250, 130, 0.3), (1024, 1, 1, 1.0), (1025, 17, 9, 0.0), (2049, 1, 1, 0.0), (2049, 250, 130, 1.0),
         (70000, 64, 48, 0.3), (70000, 64, 48, 1.0))


@pytest.mark.parametrize("N,W,H,density", ROOMS)
def test_frustum_random_rooms(N, W, H, density):
    s = R.room_scene(1000 + N + W, N, W, H, density)
    assert (s["points"] < 0).any() or N == 1
    want = _check_both_modes(s, (N, W, H, density))
    if N == 1023:   # a marker threshold other than the default
        got = M.frustum_candidates(s["points"], s["w2c"], s["K"], W, H, marker_threshold=0.0125, **R.key_args(s))
        other = R.frustum_restated(s["points"], s["w2c"], s["K"], W, H, marker_threshold=0.0125, **R.key_args(s))
        assert 0 < len(other[0]) < len(want[0])
        _assert_bit_equal(tuple(x.cpu().numpy() for x in got), other)
    if density > 0 and N >= 255 and W > 1:   # both outcomes of d < 0.1 occur
        assert 0 < len(want[0]) < int(s["mask"].sum())


def test_frustum_cell_boundaries():
    """points and keypoints on multiples of the 0.125 m grid cell, of both signs: floor() of a negative cell index, a query on
    a cell face, equal distances between different points"""
    for seed in (1, 2):
        s = R.grid_scene(seed, 3000)
        q, _ = R.backproject(s["mask"], s["depth"], s["c2w"], s["K"])
        on_face = (q * 8 == np.round(q * 8)).any(axis=1)
        assert on_face.mean() > 0.5 and (q[on_face] < 0).any()
        p = s["points"].astype(np.float64)
        assert ((p * 8 == np.round(p * 8)).all(axis=1)).mean() > 0.3
        want = _check_both_modes(s, seed)
        assert len(want[0]) > 20


def _first_kept_of_equal_rows(s):
    pz, u, v = R.project(s["points"], s["w2c"], s["K"])
    keep = (pz > 0.05) & (u >= 0) & (u < s["W"]) & (v >= 0) & (v < s["H"]) & (s["marker"] > np.float32(0.005))
    first = {}
    for i in np.flatnonzero(keep):
        first.setdefault(s["points"][i].tobytes(), i)
    return first


@pytest.mark.parametrize("kind", ("room", "grid"))
def test_frustum_duplicates_take_the_smaller_index(kind):
    """5 % of the points copied to later indices and some to earlier ones: the grid's fill order is atomic-ordered, the answer
    must not be"""
    base = R.room_scene(77, 2049, 64, 48, 1.0) if kind == "room" else R.grid_scene(5, 3000)
    s = R.with_duplicates(base, 9)
    assert len(np.unique(s["points"], axis=0)) < len(s["points"]) - 50
    want = _host_frustum(s)
    got = _device_frustum(s)
    again = _device_frustum(s)
    _assert_bit_equal(got, want, kind)
    _assert_bit_equal(again, got, kind)
    first = _first_kept_of_equal_rows(s)
    smallest = np.array([first[s["points"][i].tobytes()] for i in got[0]])
    assert np.array_equal(got[0], smallest)
    hit = sum(1 for i in np.unique(got[0]) if (s["points"] == s["points"][i]).all(axis=1).sum() > 1)
    assert hit > 0   # duplicated points are among the answers


def test_frustum_bucket_cap():
    """N above the 2^22 bucket cap: the table stops doubling and buckets share cells"""
    N = (1 << 22) + 1000
    rng = np.random.default_rng(22)
    s = R.room_scene(22, 4096, 8, 8, 1.0)
    far = rng.uniform(-20.0, 20.0, (N - 4096, 3)).astype(np.float32)
    s["points"] = np.concatenate([far[: N // 2], s["points"], far[N // 2:]])
    s["marker"] = rng.uniform(0.0, 0.02, N).astype(np.float32)
    want = _host_frustum(s)
    assert 8 < len(want[0]) < 64
    _assert_bit_equal(_device_frustum(s), want)


def _edge_camera():
    # identity pose, power-of-two intrinsics: u = (8 x + 8 z) / z and v = (8 y + 4 z) / z are exact
    return dict(w2c=np.eye(4), c2w=np.eye(4), K=np.array([[8.0, 0.0, 8.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]]), W=16, H=8)


def test_frustum_comparison_edges_of_the_projection():
    f = np.float32
    below1, above1 = np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2))
    z_hi = f(0.05)                      # 0.0500000007...: the f32 neighbour above 0.05
    z_lo = np.nextafter(z_hi, f(0))     # 0.0499999970...: the one below
    assert float(z_lo) < 0.05 < float(z_hi)
    pts = np.array([[-1, 0, 1],            # 0: u == 0 -> kept
                    [1, 0, 1],             # 1: u == W -> not
                    [below1, 0, 1],        # 2: u just below W -> kept
                    [-above1, 0, 1],       # 3: u just below 0 -> not
                    [0, -0.5, 1],          # 4: v == 0 -> kept
                    [0, 0.5, 1],           # 5: v == H -> not
                    [0, 0.5 * below1, 1],  # 6: v just below H -> kept
                    [0, -0.5 * above1, 1], # 7: v just below 0 -> not
                    [0, 0, z_hi],          # 8: z just above 0.05 -> kept
                    [0, 0, z_lo],          # 9: z just below 0.05 -> not
                    [0, 0, -1]], f)        # 10: behind the camera
    s = dict(_edge_camera(), points=pts)
    want = _host_frustum(s, key=False)
    assert want[0].tolist() == [0, 2, 4, 6, 8]
    assert want[2][0, 0] == 0.0 and want[2][2, 1] == 0.0
    _assert_bit_equal(_device_frustum(s, key=False), want)


def test_frustum_comparison_edges_of_marker_and_mask():
    f = np.float32
    cam = _edge_camera()
    W, H = cam["W"], cam["H"]
    mask = np.ones((H, W), np.int32)
    mask[0, :] = 2       # not keypoints
    mask[1, :] = -1
    # with depth 1, pixel (row, col) back-projects to ((col - 8) / 8, (row - 4) / 8, 1): neighbours are 0.125 m apart, so a
    # point placed on a pixel's position can only pair with that pixel
    thr = f(0.005)
    pts, marker = [], []
    for (r, c), mk in (((2, 3), thr),                       # 0: marker == threshold -> out
                       ((2, 5), np.nextafter(thr, f(1))),   # 1: the next f32 above -> in
                       ((0, 3), f(1)), ((1, 3), f(1)),      # 2, 3: kept points under mask values 2 and -1
                       ((3, 3), f(1))):                     # 4: the control
        pts.append([(c - 8) / 8, (r - 4) / 8, 1.0])
        marker.append(mk)
    s = dict(cam, points=np.array(pts, f), marker=np.array(marker, f), mask=mask, depth=np.ones((H, W), f))
    want = _host_frustum(s)
    assert want[0].tolist() == [1, 4]
    _assert_bit_equal(_device_frustum(s), want)
    assert _host_frustum(s, key=False)[0].tolist() == [0, 1, 2, 3, 4]
    for flat in (np.ones((H, W), np.uint8), np.ones((H, W), bool), np.ones((H, W), np.float32)):   # the mask's dtype is free
        assert _device_frustum(dict(s, mask=flat))[0].tolist() == [2, 3, 1, 4]


def test_frustum_c_abi_takes_only_mask_value_one():
    """include/splatraster.h: kp_mask == 1 is a keypoint, every other u8 value is not (the Python layer only passes 0 / 1)"""
    f = np.float32
    cam = _edge_camera()
    W, H = cam["W"], cam["H"]
    mask = np.ones((H, W), np.uint8)
    mask[0, :], mask[1, :] = 2, 255
    pts = np.array([[(3 - 8) / 8, (r - 4) / 8, 1.0] for r in (0, 1, 2)], f)   # on the back-projections of pixels (r, 3)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _native.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    p, mk, km, dp = t(pts), t(np.ones(3, f)), t(mask), t(np.ones((H, W), f))
    idx = torch.full((W * H,), -7, dtype=torch.int32, device=dev)
    xyz = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    uv = torch.empty((W * H, 2), dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.splatraster_frustum_workspace_bytes(3, W, H)), dtype=torch.uint8, device=dev)
    eye, K, kp4 = np.eye(4), cam["K"], np.array([8.0, 8.0, 8.0, 4.0])
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = lib.splatraster_frustum_candidates(3, M._ptr(p), M._ptr(mk), 0.005, hp(eye), hp(K), W, H, M._ptr(km), M._ptr(dp),
                                            hp(eye), hp(kp4), M._ptr(idx), M._ptr(xyz), M._ptr(uv), M._ptr(count), M._ptr(ws),
                                            _stream(dev))
    assert st == 0
    assert int(count.cpu()[0]) == 1 and idx.cpu().numpy()[:2].tolist() == [2, -7]


def test_frustum_radius_is_strict():
    """a distance of exactly 0.1 (the double): no pair.  The principal pixel back-projects onto (tx, ty, d + tz) exactly, and
    with tx = 0.125 - 0.1 (exact in f64) the point (0.125, 0, 1) lies ex = 0.1 away; sqrt(ex * ex) == ex in IEEE arithmetic."""
    f = np.float32
    cam = _edge_camera()
    mask = np.zeros((cam["H"], cam["W"]), np.int32)
    mask[4, 8] = 1
    tx = 0.125 - 0.1
    assert 0.125 - tx == 0.1 and np.sqrt((0.1 * 0.1 + 0.0) + 0.0) == 0.1
    t_in, t_out = 0.125 - np.nextafter(0.1, 0.0), 0.125 - np.nextafter(0.1, 1.0)   # the two f64 neighbours of 0.1, exact too
    assert 0.125 - t_in == np.nextafter(0.1, 0.0) and 0.125 - t_out == np.nextafter(0.1, 1.0)
    for t, pairs in ((tx, 0), (t_in, 1), (t_out, 0)):
        c2w = np.eye(4)
        c2w[0, 3] = t
        w2c = np.eye(4)
        w2c[0, 3] = -t
        s = dict(cam, c2w=c2w, w2c=w2c, points=np.array([[0.125, 0, 1], [3, 0, 1]], f), marker=np.ones(2, f), mask=mask,
                 depth=np.ones(mask.shape, f))
        want = _host_frustum(s)
        assert len(want[0]) == pairs and _host_frustum(s, key=False)[0].tolist() == [0]
        _assert_bit_equal(_device_frustum(s), want, t)


def test_frustum_empty_outcomes_in_both_modes():
    s = R.room_scene(5, 300, 17, 9, 1.0)
    front = R.project(s["points"], s["w2c"], s["K"])[0] > 0.05
    s["points"], s["marker"] = s["points"][front], s["marker"][front]
    empty = dict(s, points=np.zeros((0, 3), np.float32), marker=np.zeros(0, np.float32))
    away = dict(s, w2c=np.diag([1.0, -1.0, -1.0, 1.0]) @ s["w2c"])   # every point behind the camera; the keypoints stay
    blank = dict(s, mask=np.zeros_like(s["mask"]))
    for name, case, modes in (("N = 0", empty, (True, False)), ("turned away", away, (True, False)), ("mask", blank, (True,))):
        for key in modes:
            want = _host_frustum(case, key)
            assert len(want[0]) == 0, name
            idx, xyz, uv = _device_frustum(case, key)
            assert idx.shape == (0,) and xyz.shape == (0, 3) and uv.shape == (0, 2), (name, key)
    assert len(_host_frustum(s)[0]) > 0 and len(_host_frustum(blank, False)[0]) > 0


def test_frustum_depth_holes():
    """depth 0 back-projects onto the camera centre and follows the normal rule; +inf and NaN give no pair (fr_query_kernel
    searches only finite positions below 1e15, so no cell index is formed from them)"""
    s = R.room_scene(6, 1025, 17, 9, 1.0)
    depth = s["depth"].copy()
    depth[0, :6] = 0.0
    depth[1, :6] = np.inf
    depth[2, :6] = np.nan
    depth[4, 8] = np.inf    # the principal column: 0 * inf
    depth[3, 3] = np.float32(3e38)
    s["depth"] = depth
    # a kept point 0.08 m in front of the camera centre: the depth-0 pixels pair with it
    front = (s["c2w"] @ np.array([0.0, 0.0, 0.08, 1.0]))[:3]
    s["points"][0] = front.astype(np.float32)
    s["marker"][0] = 1.0
    want = _host_frustum(s)
    assert (want[0] == 0).sum() == 6
    q, ok = R.backproject(s["mask"], s["depth"], s["c2w"], s["K"])
    assert (~ok).sum() == 14
    _assert_bit_equal(_device_frustum(s), want)


def test_subset_mode_returns_the_callers_f64_rows():
    s = R.room_scene(8, 1500, 64, 48, 0.3)
    sub = s["points"].astype(np.float64)   # exactly representable in f32, as gaussian_selectition's copies are
    frame = {"w2c": torch.from_numpy(s["w2c"]), "c2w": torch.from_numpy(s["c2w"]), "K": s["K"],
             "depth": torch.from_numpy(s["depth"]), "sp_kp_mask": torch.from_numpy(s["mask"])}
    idx, _, uv = R.frustum_restated(sub, s["w2c"], s["K"], s["W"], s["H"])
    assert 0 < len(idx) < len(sub)
    p3, f3, p2 = M.get_frusm_pts(None, None, frame, s["K"], s["W"], s["H"], decoder=lambda x: x, subset=sub)
    assert p3.dtype == np.float64 and np.array_equal(p3, sub[idx]) and np.array_equal(f3.numpy(), sub[idx])
    assert np.array_equal(p2.view(np.int64), np.ascontiguousarray(uv).view(np.int64))
    p3, _, _ = M.get_frusm_pts(None, None, frame, s["K"], s["W"], s["H"], decoder=lambda x: x, subset=torch.from_numpy(sub))
    assert p3.dtype == np.float64 and np.array_equal(p3, sub[idx])


# ---- descriptor cost ------------------------------------------------------------------------------------------------
def _device_cost(d1, d2, thr):
    """splatraster_match_cost through the C ABI: the oriented [min, max] f64 matrix"""
    D, N1, N2 = d1.shape[0], d1.shape[1], d2.shape[1]
    a, b = torch.from_numpy(d1).cuda().contiguous(), torch.from_numpy(d2).cuda().contiguous()
    norms = torch.empty(N1 + N2, dtype=torch.float32, device="cuda")
    cost = torch.empty(N1 * N2, dtype=torch.float64, device="cuda")
    st = _native.load().splatraster_match_cost(D, N1, N2, M._ptr(a), M._ptr(b), float(thr), M._ptr(norms), M._ptr(cost),
                                               _stream(torch.device("cuda", torch.cuda.current_device())))
    assert st == 0
    return cost.cpu().numpy().reshape(min(N1, N2), max(N1, N2))


@pytest.mark.parametrize("D", R.COST_DIMS)
def test_cost_matrix_against_f64(D):
    """Every entry whose f64 similarity is farther than cost_bound(D) from the threshold lies within cost_bound(D) of the f64
    cost, and is exactly 1.0 below the threshold; at most 0.1 % of a case may lie inside the band.  match_sims at the assigned
    pairs equals the matrix's entries bit for bit.
    Worst observed error / bound on the MI355X (the bound is derived, (2 D + 8) * 2^-24): D = 1: 0.000, 15: 0.088,
    16: 0.099, 17: 0.097, 33: 0.080, 256: 0.024."""
    worst = 0.0
    for d, N1, N2 in R.cost_cases():
        if d != D:
            continue
        d1, d2 = R.cost_case(D, N1, N2)
        sim, want = R.cost_f64(d1, d2, R.COST_THRESHOLD)
        got = _device_cost(d1, d2, R.COST_THRESHOLD)
        band = R.band(sim, R.COST_THRESHOLD, D)
        assert band.mean() <= R.BAND_SHARE, (D, N1, N2)
        err = np.abs(got - want)[~band]
        worst = max(worst, float(err.max()) / R.cost_bound(D))
        print(f"cost D={D} N1={N1} N2={N2}: max error {err.max():.3e}, bound {R.cost_bound(D):.3e}, band {int(band.sum())}")
        assert err.max() <= R.cost_bound(D), (D, N1, N2)
        assert (got[~band & (sim < np.float32(R.COST_THRESHOLD))] == 1.0).all(), (D, N1, N2)
        inside = got[band]
        assert ((inside == 1.0) | (np.abs(inside - (1.0 - sim[band])) <= R.cost_bound(D))).all()
        # the drop-in's sims are the matrix's own entries
        m, s = M.match_descriptors(d1, d2, threshold=R.COST_THRESHOLD)
        m, s = m.cpu().numpy(), s.cpu().numpy()
        entries = got.T[m[0], m[1]] if N2 < N1 else got[m[0], m[1]]
        assert np.array_equal((np.float32(1) - s).astype(np.float64), entries), (D, N1, N2)
        r, c = lsap_restated(got.T if N2 < N1 else got)
        assert np.array_equal(m, np.stack([r, c])), (D, N1, N2)
    print(f"cost D={D}: worst error / bound {worst:.3f}")


def test_cost_directed_cases():
    d1, d2 = R.cost_case(33, 65, 130)
    d1[:, 7] = 0.0
    d2[:, 100] = 0.0
    for a, b in ((d1, d2), (d2, d1)):   # oriented rows are the 65 in both calls
        got = _device_cost(a, b, 0.4)
        assert (got[7, :] == 1.0).all() and (got[:, 100] == 1.0).all() and (got != 1.0).any()
        # threshold above every similarity: all entries exactly 1, the constant matrix gives the identity assignment
        assert (_device_cost(a, b, 1.5) == 1.0).all()
        m, s = M.match_descriptors(a, b, threshold=1.5)
        k = np.arange(65)
        assert np.array_equal(m.cpu().numpy(), np.stack([k, k])) and (s.cpu().numpy() == 0).all()
        # threshold below every similarity: nothing is zeroed
        sim, want = R.cost_f64(a, b, -2.0)
        assert np.array_equal(want, 1.0 - sim)
        assert np.abs(_device_cost(a, b, -2.0) - want).max() <= R.cost_bound(33)
    # D = 1: every normalised element is exactly +-1 (sqrt(x * x) == |x| and x / |x| == +-1 in IEEE arithmetic), so a
    # similarity of 1 sits exactly on a threshold of 1.0: `sim < thr` is false there and the pair keeps its cost of 0
    d1, d2 = R.cost_case(1, 63, 65)
    agree = np.sign(d1[0])[:, None] == np.sign(d2[0])[None, :]
    assert agree.any() and not agree.all()
    assert np.array_equal(_device_cost(d1, d2, 1.0), np.where(agree, 0.0, 1.0))


# ---- solver ---------------------------------------------------------------------------------------------------------
def _np(pair):
    return tuple(x.cpu().numpy() for x in pair)


def _scipy():
    try:
        from scipy.optimize import linear_sum_assignment
        return linear_sum_assignment
    except ImportError:
        return None


def _family(rng, shape, kind):
    if kind == "ties":
        return rng.integers(0, 3, size=shape).astype(np.float64)
    if kind == "contested":   # every row wants the same few columns: long augmenting paths, quarter-valued ties
        return rng.integers(0, 40, size=(1, shape[1])) / 4.0 + rng.integers(0, 3, size=shape) / 4.0
    if kind == "signed":      # negative, mixed-sign and -0.0 entries
        c = rng.integers(-3, 4, size=shape) / 2.0
        c[rng.random(shape) < 0.2] = -0.0
        return c
    if kind == "negative":
        return -rng.random(shape) - rng.integers(0, 3, size=shape)
    if kind == "extreme":     # 1e-300 and 1e300 in one matrix
        c = rng.choice(np.array([1e-300, 2e-300, 1e300, 3e300, 0.0, 1.0]), size=shape)
        return c
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _solver_case(shape, kind, seed=0):
    """(cost, rows, cols, steps) with the restatement's answer, checked against scipy's where it can be imported; computed
    once"""
    c = _family(np.random.default_rng(seed + shape[0] * 7 + shape[1]), shape, kind)
    r, cc, steps = lsap_restated(c, return_steps=True)
    lsa = _scipy()
    if lsa is not None:
        sr, sc = lsa(c)
        assert np.array_equal(r, sr) and np.array_equal(cc, sc), (shape, kind)
    return c, r, cc, steps


BOUNDARY = tuple(s for nc in (1024, 1025, 4096, 4097) for s in ((37, nc), (nc, 37)))


@pytest.mark.parametrize("shape", BOUNDARY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver_at_the_variant_boundaries(shape):
    for kind in ("ties", "contested", "signed"):
        c, r, cc, steps = _solver_case(shape, kind)
        gr, gc, gs = M.linear_sum_assignment(c, return_steps=True)
        assert np.array_equal(gr.cpu().numpy(), r) and np.array_equal(gc.cpu().numpy(), cc), (shape, kind)
        assert gs == steps, (shape, kind)   # the same Dijkstra steps, not only the same answer


SQUARE = ((257, 257), (1024, 1024))


@pytest.mark.parametrize("shape", SQUARE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver_square_lds_path(shape):
    for kind in ("ties", "contested", "signed"):
        c, r, cc, steps = _solver_case(shape, kind)
        gr, gc, gs = M.linear_sum_assignment(c, return_steps=True)
        assert np.array_equal(gr.cpu().numpy(), r) and np.array_equal(gc.cpu().numpy(), cc), (shape, kind)
        assert gs == steps, (shape, kind)   # the same Dijkstra steps, not only the same answer


@pytest.mark.parametrize("shape", SQUARE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver_square_global_path(shape, global_path):  # noqa: F811
    for kind in ("ties", "contested", "signed"):
        c, r, cc, steps = _solver_case(shape, kind)
        gr, gc, gs = M.linear_sum_assignment(c, return_steps=True)
        assert np.array_equal(gr.cpu().numpy(), r) and np.array_equal(gc.cpu().numpy(), cc), (shape, kind)
        assert gs == steps, (shape, kind)   # the same Dijkstra steps, not only the same answer


def test_solver_cost_families():
    for shape in ((40, 90), (90, 40), (64, 64), (5, 1100)):
        for kind in ("ties", "signed", "negative", "extreme"):
            c, r, cc, steps = _solver_case(shape, kind, seed=3)
            gr, gc, gs = M.linear_sum_assignment(c, return_steps=True)
            assert np.array_equal(gr.cpu().numpy(), r) and np.array_equal(gc.cpu().numpy(), cc), (shape, kind)
            assert gs == steps, (shape, kind)
    # maximize on f32 input that is inexact in decimal: widened exactly, negated, solved in f64
    rng = np.random.default_rng(12)
    lsa = _scipy()
    for shape in ((30, 70), (70, 30), (50, 50)):
        c32 = (rng.random(shape) * rng.choice([0.1, 1.0, 10.0], size=shape)).astype(np.float32)
        r, cc = lsap_restated(c32.astype(np.float64), maximize=True)
        if lsa is not None:
            sr, sc = lsa(c32, maximize=True)
            assert np.array_equal(r, sr) and np.array_equal(cc, sc)
        for arg in (c32, torch.from_numpy(c32).cuda()):
            gr, gc = _np(M.linear_sum_assignment(arg, maximize=True))
            assert np.array_equal(gr, r) and np.array_equal(gc, cc), shape


def test_solver_at_the_16_bit_index_limit():
    n = M.MAX_NC
    assert n == 65535
    for nr in (1, 3):
        for col in (n - 1, 0):
            c = np.full((nr, n), 2.0)
            c[nr - 1, col] = 1.0   # the unique minimum, in the last row
            gr, gc = _np(M.linear_sum_assignment(c))
            r, cc = lsap_restated(c)
            assert gc[nr - 1] == col and len(set(gc.tolist())) == nr
            assert np.array_equal(gr, r) and np.array_equal(gc, cc), (nr, col)
        gr, gc = _np(M.linear_sum_assignment(np.full((nr, n), 0.5)))
        assert np.array_equal(gr, np.arange(nr)) and np.array_equal(gc, np.arange(nr))
    rng = np.random.default_rng(2)
    c = rng.integers(0, 4, size=(n, 2)).astype(np.float64)   # the transposed form
    c[n - 1, 0] = -1.0
    c[0, 1] = -1.0
    gr, gc = _np(M.linear_sum_assignment(c))
    r, cc = lsap_restated(c)
    assert np.array_equal(gr, r) and np.array_equal(gc, cc)
    assert gr.tolist() == [0, n - 1] and gc.tolist() == [1, 0]


def _abi_batch(mats):
    """splatraster_lsap on a batch through the C ABI, without the Python layer's raise: (rows, cols, status, offsets)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    pieces, problems, offs, off, total = [], [], [], 0, 0
    for c in mats:
        flat, tr = M._orient(torch.from_numpy(np.ascontiguousarray(c)), dev)
        pieces.append(flat)
        problems.append(M.LsapProblem(off, min(c.shape), max(c.shape), int(tr), 0))
        off += flat.numel()
        offs.append(total)
        total += min(c.shape)
    B = len(mats)
    table = (M.LsapProblem * B)(*problems)
    lib = _native.load()
    rows = torch.full((total,), -7, dtype=torch.int64, device=dev)
    cols = torch.full((total,), -7, dtype=torch.int64, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    steps = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.splatraster_lsap_workspace_bytes(B, table)), 1), dtype=torch.uint8, device=dev)
    costs = torch.cat(pieces)
    st = lib.splatraster_lsap(B, table, M._ptr(costs), 0, M._ptr(rows), M._ptr(cols), M._ptr(status), M._ptr(steps), M._ptr(ws),
                              _stream(dev))
    assert st == 0
    return rows.cpu().numpy(), cols.cpu().numpy(), status.cpu().numpy(), offs


def test_batch_status_per_problem():
    rng = np.random.default_rng(65)
    mats = [rng.integers(0, 5, size=(int(rng.integers(1, 30)), int(rng.integers(1, 30)))) / 4.0 for _ in range(65)]
    mats[11] = mats[11].copy()
    mats[11].flat[mats[11].size // 2] = np.nan
    mats[40] = np.full((3, 6), 1.0)
    mats[40][1, :] = np.inf   # infeasible
    rows, cols, status, offs = _abi_batch(mats)
    want = np.zeros(65, np.int32)
    want[11], want[40] = M.LSAP_INVALID, M.LSAP_INFEASIBLE
    assert np.array_equal(status, want)
    for k, c in enumerate(mats):
        if k in (11, 40):
            continue
        n = min(c.shape)
        r, cc = _np(M.linear_sum_assignment(c))
        assert np.array_equal(rows[offs[k]:offs[k] + n], r) and np.array_equal(cols[offs[k]:offs[k] + n], cc), k
        hr, hc = lsap_restated(c)
        assert np.array_equal(r, hr) and np.array_equal(cc, hc), k
    with pytest.raises(ValueError, match="invalid numeric entries"):
        M.linear_sum_assignment_batch(mats)
    with pytest.raises(ValueError, match="infeasible"):
        M.linear_sum_assignment_batch(mats[12:])


def test_batch_sizes_around_one_launch_chunk():
    """exactly 64, 65 and 128 problems of one kernel variant (64 per launch)"""
    rng = np.random.default_rng(128)
    mats = [rng.integers(0, 4, size=(int(rng.integers(1, 40)), int(rng.integers(1, 40)))).astype(np.float64)
            for _ in range(128)]
    single = [_np(M.linear_sum_assignment(c)) for c in mats]
    for c, (r, cc) in zip(mats[:40], single):
        hr, hc = lsap_restated(c)
        assert np.array_equal(r, hr) and np.array_equal(cc, hc)
    for B in (64, 65, 128):
        out = M.linear_sum_assignment_batch(mats[:B])
        assert len(out) == B
        for k, ((r, cc), (sr, sc)) in enumerate(zip(out, single)):
            assert np.array_equal(r.cpu().numpy(), sr) and np.array_equal(cc.cpu().numpy(), sc), (B, k)


def _batch_equals_single(mats, maximize=False):
    out = M.linear_sum_assignment_batch(mats, maximize=maximize)
    assert len(out) == len(mats)
    for k, (c, (r, cc)) in enumerate(zip(mats, out)):
        sr, sc = _np(M.linear_sum_assignment(c, maximize=maximize))
        hr, hc = lsap_restated(c, maximize)
        assert np.array_equal(sr, hr) and np.array_equal(sc, hc), k
        assert np.array_equal(r.cpu().numpy(), hr) and np.array_equal(cc.cpu().numpy(), hc), k


def test_batch_members_in_the_global_workspace():
    """more than one member beyond 4096 columns: each has its own slice of the workspace"""
    rng = np.random.default_rng(41)
    shapes = ((20, 4100), (7, 9), (5000, 12), (33, 4097), (40, 1100), (3, 65535))
    _batch_equals_single([_family(rng, s, "contested") for s in shapes])
    _batch_equals_single([_family(rng, s, "signed") for s in shapes[:5]], maximize=True)


def test_batch_under_the_global_path(global_path):  # noqa: F811
    rng = np.random.default_rng(42)
    mats = [_family(rng, (int(rng.integers(1, 40)), int(rng.integers(1, 40))), "ties") for _ in range(66)]
    _batch_equals_single(mats)
