"""Host side of the grid-encoding edge tests (tests/test_gpu_grid_encoding_edges.py): every named layout of
tests/grid_encoding_reference.py is accepted and has the property its builder names, every point builder reaches its edge at
every level, the exact family stays inside the magnitudes that keep float32 exact, the float32 model of the kernels (`model32`)
meets every check the device tests make and each of its deliberate defects fails the check named for it here, and the C
entries refuse bad arguments before any launch.  No GPU needed.

Measured with the model, worst |model - float64| / bar over the bounded layouts and batch sizes: forward 0.55 (L32, N = 777),
table gradient 0.024 (L32, N = 777), input gradient 0.0084 (flat, N = 777); every exact case equal to the float64 restatement."""
import ctypes

import pytest
import torch

from tests import grid_encoding_reference as R


def _run(wrong=None):
    return lambda x, p, lay, G, want: R.model32(x, p, lay, G, want, wrong)


def test_every_named_layout_is_accepted_and_has_its_property():
    for name, (D, cfg, edge) in R.LAYOUTS.items():
        lay = R.layout(name)                       # raises if the host layout call refuses it
        assert edge and lay.n_input_dims == D and lay.n_levels == cfg["n_levels"]
        assert lay.n_params == sum(lay.sizes) * lay.n_features_per_level
    assert sorted((R.layout(n).n_input_dims, R.layout(n).n_features_per_level) for n in R.EXACT if n.startswith("int6_hash")) == \
        [(D, F) for D in (2, 3) for F in (1, 2, 4, 8)]
    for name in R.EXACT:
        lay = R.layout(name)
        if name.startswith("int6"):
            assert lay.scales == [0.0, 1.0, 3.0, 7.0, 15.0, 31.0] and lay.resolutions[0] == 1 and R.lanes_per_point(lay) == 8
        if name.startswith("int6_tiled"):
            assert lay.sizes == [1] * 6 and lay.n_params == 6 * lay.n_features_per_level
        if name.startswith("int6_hash"):
            assert R.hashed_levels(lay) == [False] * 3 + [True] * 3
        if name.startswith("int6_dense"):
            assert all(s >= r ** lay.n_input_dims for s, r in zip(lay.sizes, lay.resolutions))
    for name, res, size in (("eq3", 4, 16), ("eq2", 8, 8)):
        lay = R.layout(name)
        assert lay.resolutions[0] == res and lay.sizes[0] == size and R.stride_meets_size(lay, 0) and R.hashed_levels(lay)[0]
    for name, D in (("tiled5", 3), ("tiled5_2", 2)):
        lay = R.layout(name)
        assert lay.sizes == [5 ** D] * 4 and lay.offsets == [0, 5 ** D, 2 * 5 ** D, 3 * 5 ** D] and lay.offsets[1] % 2 == 1
        assert [r ** D > s for r, s in zip(lay.resolutions, lay.sizes)] == [False, True, True, True]      # levels that wrap
    assert R.layout("tiled5").sizes == [125, 125, 125, 125]
    assert [R.lanes_per_point(R.layout(n)) for n in ("one_level", "two", "three", "L17", "L32")] == [1, 2, 4, 32, 32]
    assert R.layout("L17").n_levels == 17 and R.layout("L32").n_levels == 32 and R.layout("L32").n_output_dims == 256
    assert any(R.hashed_levels(R.layout("L32"))) and not all(R.hashed_levels(R.layout("L32")))
    assert len(set(R.layout("flat").scales)) == 1 and R.layout("flat").scales[0] == 6.0
    s = R.layout("shrinking").scales
    assert all(a > b for a, b in zip(s, s[1:])) and any(R.hashed_levels(R.layout("shrinking")))
    assert R.layout("one_level").scales == [16.0]
    for name in R.BOUNDED:
        lay = R.layout(name)
        per_group = 256 // R.lanes_per_point(lay)
        assert R.batch_sizes(lay) == [1, per_group - 1, per_group, per_group + 1, 777]


def test_every_point_builder_reaches_its_edge():
    """per level of every layout: points with a frac of exactly 0 and points with a negative cell are in every batch of 64 or more
    (at some level in the smaller ones, which also hold 0, 1 and outside points); points in eighths give an exact pos at every
    integer scale"""
    for name in R.EXACT:
        lay = R.layout(name)
        for n in (R.EXACT_N, R.ROWS_N):
            x = R.case(name, n)[0]
            assert float(x.min()) == -1.0 and float(x.max()) == 2.0 and bool((x * 8 == torch.round(x * 8)).all())
            for lvl, (faces, negative, exact) in enumerate(R.cell_census(x, lay)):
                assert exact, (name, lvl)
                assert (faces > 0 and negative > 0) or lay.scales[lvl] == 0, (name, lvl)       # scale 0: every pos is 0.5
    for name in R.BOUNDED:
        lay = R.layout(name)
        for n in R.batch_sizes(lay):
            x = R.case(name, n)[0]
            assert x.shape == (n, lay.n_input_dims)
            if n == 1:
                continue
            census = R.cell_census(x, lay)
            every = all if n >= 64 else any           # a batch of 7 has two face rows: not one for each of 32 levels
            assert every(negative > 0 for _, negative, _ in census), (name, n, census)
            assert every(faces > 0 for faces, _, _ in census), (name, n, census)
            assert bool((x == 0).any()) and bool((x == 1).any()) and float(x.min()) < 0 and (float(x.max()) > 1 or n < 64)
    pool = R.points(R.SMALL_POOL, 1, R.layout("L32"))
    assert torch.equal(R.bounded_points(7, 1, R.layout("L32")), pool[[0, 192, 64, 128, 200, 1, 193]])


@pytest.mark.parametrize("name", list(R.EXACT))
def test_exact_family_stays_exact(name):
    """the two magnitude conditions, on the float64 restatement: sum of |terms| per table entry below 2^13, the input gradient's
    bound below 2^15; outputs and both gradients round-trip through float32 unchanged; the model equals them"""
    ref = R.reference(name)
    assert float(ref["dparams_abs"].max()) < R.EXACT_TERMS_BELOW and float(ref["dx_bound"].max()) < R.EXACT_DX_BELOW
    for k in ("out", "dparams", "dx"):
        assert torch.equal(ref[k].float().double(), ref[k]), k
        # a table of one entry per level encodes a constant: its input gradient is the exact cancellation of equal terms
        assert float(ref[k].abs().max()) > 0 or (k == "dx" and name.startswith("int6_tiled"))
    assert bool((ref["out"] * 2 ** 9 == torch.round(ref["out"] * 2 ** 9)).all())
    assert R.check_exact(_run(), name) == []
    for want in (("out",), ("dparams",), ("dx",)):            # the three backward kernels compute the same numbers
        assert R.check_exact(_run(), name, want=want) == []


@pytest.mark.parametrize("name", list(R.BOUNDED))
def test_the_model_meets_the_three_bars(name):
    worst = {}
    for n in R.batch_sizes(R.layout(name)):
        r = R.check_bounded(_run(), name, n)
        assert R.within(r), (name, n, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        ref = R.reference(name, n)
        assert float(ref["dx"].abs().max()) > 0 and int((ref["dparams_abs"] > 0).sum()) > 0
    print(f"{name}: worst |model - float64| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("name,n", [("L17", 777), ("L32", 9), ("one_level", 1)])
@pytest.mark.parametrize("what", ["dx", "dparams", "out"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_nan_or_inf_anywhere_fails_the_bars(name, n, what, value):
    """one NaN or infinity planted in the model's output or either gradient fails that result's bar (and no other), also in a
    table entry nothing contributes to, whose bar is 0; planted in an exact case it fails the exact comparison"""
    x, p, G = R.case(name, n)
    ref = R.reference(name, n)
    got = {k: v.clone() for k, v in R.model32(x, p, R.layout(name), G).items()}
    assert R.within(R.ratios(got, ref))
    spot = int(torch.nonzero(ref["dparams_abs"] == 0)[0]) if what == "dparams" else 0
    got[what].view(-1)[spot] = value
    r = R.ratios(got, ref)
    assert r[what] == float("inf") and not R.within(r) and [k for k, v in r.items() if not v <= 1.0] == [what]
    exact = {k: v.clone() for k, v in R.model32(*R.case("eq2")[:2], R.layout("eq2"), R.case("eq2")[2]).items()}
    exact[what].view(-1)[0] = value
    assert R.inexact(exact, R.reference("eq2")) == [what]


@pytest.mark.parametrize("name", R.ROWS_LAYOUTS)
def test_the_model_s_rows_are_independent(name):
    assert R.check_rows(_run(), name) == []


def test_the_model_s_collisions_add_up():
    for name in R.COLLISION_LAYOUTS:
        assert R.check_collisions(_run(), name) == []


# defect: the checks that catch it, (check, layout, batch size), the first being the case named for it
EXPOSED_BY = {
    "stride_lt": [("exact", "eq2", None), ("exact", "eq3", None), ("bars", "tiled5_2", 777)],
    "hash_le": [("exact", "int6_hash_d2f1", None), ("exact", "int6_hash_d3f4", None)],
    "primes_swapped": [("exact", "int6_hash_d3f1", None), ("bars", "two", 777)],
    "no_wrap": [("bars", "tiled5", 777), ("bars", "tiled5_2", 63)],
    "trunc": [("exact", "int6_dense_d2f1", None), ("bars", "tiled5", 777)],
    "no_half": [("exact", "int6_dense_d3f2", None), ("bars", "one_level", 1)],
    "clamp": [("exact", "int6_dense_d3f2", None), ("bars", "L17", 777)],
    "weight_swapped": [("exact", "int6_dense_d2f2", None), ("bars", "two", 1)],
    "corner_bit_reversed": [("exact", "int6_dense_d3f1", None), ("bars", "three", 63)],
    "feature_major": [("exact", "int6_hash_d3f2", None), ("bars", "L32", 9)],
    "offset_no_F": [("exact", "int6_tiled_d2f2", None), ("bars", "tiled5", 64)],
    "first4": [("exact", "int6_hash_d2f8", None), ("exact", "int6_tiled_d3f8", None), ("bars", "three", 65)],
    "dx_sign": [("exact", "int6_hash_d3f2", None), ("bars", "one_level", 256)],
    "dx_no_scale": [("exact", "int6_hash_d2f4", None), ("bars", "flat", 64)],
    "dx_pow2_levels": [("exact", "int6_hash_d3f2", None), ("bars", "L17", 8), ("bars", "three", 1)],
    "dx_2lp": [("rows", "int6_hash_d3f2", None), ("rows", "L32", None), ("exact", "int6_dense_d2f1", None)],
    "dp_store": [("collisions", "int6_tiled_d3f2", None), ("collisions", "eq2", None), ("exact", "int6_tiled_d2f1", None)],
}


def _fails(wrong, check, name, n):
    if check == "exact":
        return R.check_exact(_run(wrong), name)
    if check == "bars":
        return [k for k, v in R.check_bounded(_run(wrong), name, n).items() if not v <= 1.0]
    if check == "rows":
        return R.check_rows(_run(wrong), name, sample=8)
    return R.check_collisions(_run(wrong), name)


@pytest.mark.parametrize("wrong", list(R.WRONG))
def test_every_defect_fails_the_checks_named_for_it(wrong):
    assert set(EXPOSED_BY) == set(R.WRONG)
    for check, name, n in EXPOSED_BY[wrong]:
        failed = _fails(wrong, check, name, n)
        print(f"{wrong} ({R.WRONG[wrong]}): {check} {name}{'' if n is None else ' N = %d' % n} fails {failed}")
        assert failed, (wrong, check, name, n)
        assert _fails(None, check, name, n) == []


def test_first4_and_pow2_defects_touch_only_what_they_name():
    """a defect that a case cannot show is equal to the model there: first4 below F = 8, the level count of a power of two"""
    assert R.check_exact(_run("first4"), "int6_hash_d3f4") == []
    assert R.within(R.check_bounded(_run("dx_pow2_levels"), "L32", 9))


# ---- the C entries' argument checks: they return before any launch -------------------------------------------------------

BAD_ARG = 1
# An aligned and a misaligned made-up address.  Never dereferenced while the argument checks return before any launch, which is
# what these tests pin.  This file also runs where a device is present: should such a check ever regress, the entry would launch
# a kernel on these addresses there, so mend the check first and do not re-run the failing test on a device to look at it.
A, OFF = 0x10000, 0x10004


def _entries():
    from splatloc_amd import _native
    lib = _native.load()
    lay = _native.GridLayout()
    assert lib.splatraster_grid_encoding_layout(3, 4, 2, 19, 5, 1.7, _native.GRID_TILED, ctypes.byref(lay)) == 0
    return lib, lay


def _copy(lay):
    c = type(lay)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(lay), ctypes.sizeof(lay))
    return c


def test_c_entries_refuse_misaligned_pointers():
    lib, lay = _entries()
    fwd, bwd = lib.splatraster_grid_encoding_forward, lib.splatraster_grid_encoding_backward
    assert fwd(ctypes.byref(lay), 1, A, OFF, A, None) == BAD_ARG                 # params
    assert fwd(ctypes.byref(lay), 1, A, A, OFF, None) == BAD_ARG                 # out
    assert bwd(ctypes.byref(lay), 1, A, A, OFF, A, A, None) == BAD_ARG           # dL_dout
    assert bwd(ctypes.byref(lay), 1, A, A, OFF, A, None, None) == BAD_ARG
    assert bwd(ctypes.byref(lay), 1, A, A, OFF, None, A, None) == BAD_ARG
    assert bwd(ctypes.byref(lay), 1, A, OFF, A, None, A, None) == BAD_ARG        # params, read for dL_dx
    assert bwd(ctypes.byref(lay), 1, A, A, A, OFF, None, None) == BAD_ARG        # dL_dparams
    assert fwd(ctypes.byref(lay), 1, None, A, A, None) == BAD_ARG and bwd(ctypes.byref(lay), 1, A, None, A, None, A, None) == BAD_ARG


def test_c_entries_refuse_inconsistent_layouts_and_negative_n():
    lib, lay = _entries()
    fwd, bwd = lib.splatraster_grid_encoding_forward, lib.splatraster_grid_encoding_backward

    def both(bad, n=1):
        assert fwd(ctypes.byref(bad), n, A, A, A, None) == BAD_ARG
        assert bwd(ctypes.byref(bad), n, A, A, A, A, A, None) == BAD_ARG

    assert list(lay.offset[:4]) == [0, 125, 250, 375] and lay.n_params == 1000
    bad = _copy(lay)
    bad.offset[2] = 256                                # not the running sum of the sizes
    both(bad)
    bad = _copy(lay)
    bad.offset[0] = 1
    both(bad)
    bad = _copy(lay)
    bad.n_params = 1008
    both(bad)
    bad = _copy(lay)
    bad.n_params = 500                                 # the entry count, not times F
    both(bad)
    bad = _copy(lay)
    bad.size[3] = 0
    bad.n_params = 750
    both(bad)
    both(lay, -1)
    both(lay, -2 ** 40)
    assert fwd(ctypes.byref(lay), 0, None, None, None, None) == 0                # an empty batch needs no pointers
    assert bwd(ctypes.byref(lay), 0, None, None, None, None, None, None) == 0
    assert bwd(ctypes.byref(lay), 1, None, None, None, None, None, None) == 0   # nothing asked for: nothing done
