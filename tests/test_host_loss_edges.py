"""tests/loss_reference.py pinned on the host: the seeded builders reproduce the inputs tests/golden/loss_edges.npz was recorded from, the
reference's float32 results lie where the float64 oracle (oracle/losses.py) puts them (which pins the oracle's tie rules to the
reference's), every case reaches the edge it is named for, and every wrong model deviates from the oracle by more than the case's
bound, so that the device tests of tests/test_gpu_loss_edges.py cannot pass vacuously.  The argument checks of the loss entry points
of the C ABI run here too: they return before any HIP call.  No test here touches a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import losses as OL
from tests import loss_reference as R

F32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden", "loss_edges.npz")
CANCELLING = ("content smooth_converged", "content flat_offset")     # sigma = E[x^2] - mu^2 cancels in the reference's float32


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _oracle_mapping(c, ex):
    return OL.mapping_loss(*R.mapping_inputs(c), float(R.THR), *(ex if ex is not None else (None, None)))


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_builders_reproduce_the_recorded_inputs(gold):
    for name in R.refine_case_names():
        c = R.refine_case(name)
        assert np.array_equal(R.checksum(c["image"], c["gt"]), gold[f"refine__{name}__checksum"]), name
    for name in R.eval_case_names():
        c = R.eval_case(name)
        assert np.array_equal(R.checksum(c["render"], c["gt"]), gold[f"eval__{name}__checksum"]), name
    for name in R.mapping_case_names():
        assert np.array_equal(R.checksum(*R.mapping_inputs(R.mapping_case(name))), gold[f"mapping__{name}__checksum"]), name
    assert not any("grid stride" in k for k in gold.files)           # oracle only
    assert os.path.getsize(GOLD) < 1_000_000
    assert all(gold[k].dtype.kind in "fu" for k in gold.files)       # data only


def test_models_without_a_defect_are_the_oracle():
    c = R.refine_case("shape 3x17x33")
    for lam in R.LAMBDAS:
        o, m = OL.refinement_loss(c["image"], c["gt"], lam), R.refine_model(c["image"], c["gt"], lam)
        assert all(abs(o[k] - m[k]) <= 1e-14 for k in ("l1", "ssim", "loss"))
        assert np.abs(o["dL_dimage"] - m["dL_dimage"]).max() <= 1e-14 * np.abs(o["dL_dimage"]).max()
    e = R.eval_case("shape 3x17x17")
    o, m = OL.eval_metrics(e["render"], e["gt"]), R.eval_model(e["render"], e["gt"])
    assert o["count"] == m["count"] and o["mse"] == m["mse"] and o["psnr"] == m["psnr"] and abs(o["ssim"] - m["ssim"]) <= 1e-14
    for name in ("hw 257", "rgb ties", "marker saturation"):
        mc = R.mapping_case(name)
        for ex in R.EXPOSURES.values():
            o, m = _oracle_mapping(mc, ex), R.mapping_model(mc, ex)
            assert all(np.array_equal(np.asarray(o[k]), np.asarray(m[k])) for k in o), name


@pytest.mark.parametrize("name", R.refine_case_names())
def test_refinement_fixture_against_oracle(gold, name):
    """the tolerances of tests/test_oracle_losses.py; where the reference's float32 variance cancels (image ~ gt, smooth and bright) its
    SSIM map is only good to 1e-3 of itself, which is what makes that regime a case of its own"""
    c = R.refine_case(name)
    for lam in R.LAMBDAS:
        o = OL.refinement_loss(c["image"], c["gt"], lam)
        l1, ssim, loss = (float(v) for v in gold[f"refine__{name}__lam{lam}__terms"])
        ref = gold[f"refine__{name}__lam{lam}__grad"].astype(np.float64)
        assert ref.shape == c["image"].shape
        rel = 1e-3 if name in CANCELLING else 5e-6
        assert abs(o["l1"] - l1) <= 2e-6 * l1 and abs(o["ssim"] - ssim) <= rel * ssim
        assert abs(o["loss"] - loss) <= (1 - lam) * 2e-6 * l1 + lam * rel * ssim + 1e-12
        if name == "content black":
            assert l1 == 0 and ssim == 1 and not ref.any() and not o["dL_dimage"].any() and o["ssim"] == 1.0
        elif name == "content flat_equal":
            assert l1 == 0 and np.abs(ref - o["dL_dimage"]).max() <= max(R.flat_equal_grad_bound(c["image"], c["gt"], lam), 0.0)
        else:
            assert np.abs(o["dL_dimage"] - ref).max() <= (1e-3 if name in CANCELLING else 2e-4) * np.abs(ref).max()
            assert np.array_equal(ref == 0, o["dL_dimage"] == 0) or lam != 0.0       # at lambda 0 the gradient is sign / n: same zeros


@pytest.mark.parametrize("name", R.eval_case_names())
def test_eval_fixture_against_oracle(gold, name):
    c = R.eval_case(name)
    o = OL.eval_metrics(c["render"], c["gt"])
    psnr, ssim, mse, count = gold[f"eval__{name}__out"]
    assert o["count"] == int(count)                                  # the subnormal gt counts, the exact zeros do not
    assert abs(o["ssim"] - ssim) <= 1e-5
    if name == "empty mask":
        assert np.isnan(psnr) and np.isnan(mse) and np.isnan(o["psnr"]) and count == 0
    elif name == "identical":
        assert np.isposinf(psnr) and mse == 0 and np.isposinf(o["psnr"]) and o["mse"] == 0
    else:
        assert abs(o["psnr"] - psnr) <= 2e-5 * abs(psnr) and abs(o["mse"] - mse) <= 2e-6 * mse


@pytest.mark.parametrize("name", R.mapping_case_names())
def test_mapping_fixture_against_oracle(gold, name):
    """the tolerances of tests/test_oracle_losses.py, and the same exact zeros: the masks' tie rules are the reference's"""
    c = R.mapping_case(name)
    for ex_name, ex in R.EXPOSURES.items():
        o = _oracle_mapping(c, ex)
        pre = f"mapping__{name}__{ex_name}__"
        lm, bce = (float(v) for v in gold[pre + "loss"])
        assert abs(o["loss_rgbd"] - lm) <= 2e-6 * abs(lm) and abs(o["loss_bce"] - bce) <= 2e-6 * abs(bce)
        for k, ok in (("g_image", "dL_dimage"), ("g_depth", "dL_ddepth"), ("g_marker", "dL_dmarker")):
            ref = gold[pre + k].astype(np.float64)
            want = np.asarray(o[ok]).reshape(ref.shape)
            assert np.abs(want - ref).max() <= 2e-6 * np.abs(ref).max() + 1e-12, (ex_name, k)
            if k != "g_marker":
                assert np.array_equal(ref == 0, want == 0), (ex_name, k)
        assert R.ulps_apart(gold[pre + "g_depth"], o["dL_ddepth"].astype(F32).reshape(gold[pre + "g_depth"].shape)).max() <= R.G_DEPTH_ULPS
        assert R.ulps_apart(gold[pre + "g_image"], o["dL_dimage"].astype(F32).reshape(gold[pre + "g_image"].shape)).max() <= R.G_IMAGE_ULPS
        ga, gb = (float(v) for v in gold[pre + "g_exposure"])
        assert abs(o["dL_dexposure_a"] - ga) <= 1e-5 * abs(ga) + 1e-12 and abs(o["dL_dexposure_b"] - gb) <= 1e-5 * abs(gb) + 1e-12
        assert (ex is None) == (ga == 0 and gb == 0)
    # a = b = 0 with the pair present changes no value and no image gradient
    for k in ("loss", "g_image", "g_depth", "g_marker"):
        assert np.array_equal(gold[f"mapping__{name}__none__{k}"], gold[f"mapping__{name}__zero__{k}"])


# ---- every case reaches the edge it names ---------------------------------------------------------------------------------------------
def test_case_lists_hold_what_the_issue_lists():
    assert set(R.REFINE_SHAPES) >= {(1, 1, 1), (1, 5, 5), (3, 6, 6), (3, 16, 32), (3, 17, 33), (3, 15, 31), (1, 16, 37), (3, 21, 43),
                                    (3, 1400, 1), (3, 1, 2752)} and any(s[0] == 4 for s in R.REFINE_SHAPES)
    assert R.CONTENTS == ("noise", "smooth_converged", "flat_offset", "flat_equal", "black", "l1_ties") and R.CONTENT_SHAPE == (3, 37, 53)
    assert R.LAMBDAS == (0.2, 1.0, 0.0)
    assert R.EVAL_SHAPES == ((3, 33, 47), (1, 1, 1), (3, 16, 16), (3, 17, 17), (1, 5, 40))
    assert R.MAPPING_HW == (1, 63, 64, 255, 256, 257, 4801) and R.GRID_STRIDE_HW == 2048 * 256 + 257
    assert set(R.LOGITS) == {0.0, 16.6, -16.6, 17.0, -17.0, 88.0, -88.0, 89.0, -89.0, 1e4, -1e4} and R.SOFT_TARGETS == (0.0, 1.0, 1e-6, 0.999)
    assert R.MARGIN == 4.0 and (R.FW, R.FH, R.ET, R.RH, R.BLOCK) == (32, 16, 16, 5, 256)


def test_refinement_shapes_reach_their_tile_edges():
    #        shape: tiles down, tiles across, rows of the last tile, columns of the last tile, blocks
    want = {(1, 1, 1): (1, 1, 1, 1, 1), (1, 5, 5): (1, 1, 5, 5, 1), (3, 6, 6): (1, 1, 6, 6, 3), (3, 16, 32): (1, 1, 16, 32, 3),
            (3, 17, 33): (2, 2, 1, 1, 12), (3, 15, 31): (1, 1, 15, 31, 3), (1, 16, 37): (1, 2, 16, 5, 2), (3, 21, 43): (2, 2, 5, 11, 12),
            (3, 1400, 1): (88, 1, 8, 1, 264), (3, 1, 2752): (1, 86, 1, 32, 258), (4, 17, 33): (2, 2, 1, 1, 16)}
    assert set(want) == set(R.REFINE_SHAPES)
    for shape, (ty, tx, lr, lc, blocks) in want.items():
        e = R.refine_case(R.shape_name(shape))["edge"]
        assert (e["tiles"], e["last_rows"], e["last_cols"], e["blocks"]) == ((ty, tx), lr, lc, blocks), shape
    # more than 256 blocks: refine_finish_block's stride loop takes a second round, with a ragged one (264 = 256 + 8, 258 = 256 + 2)
    assert [b for b in (want[s][4] for s in R.REFINE_SHAPES) if b > R.BLOCK] == [264, 258, ]
    # (1,5,5): the window of EVERY pixel overhangs the image on all four sides; (3,6,6): a corner's window ends on the far edge exactly
    C_, H, W = 1, 5, 5
    assert all(y - R.RH < 0 and y + R.RH >= H and x - R.RH < 0 and x + R.RH >= W for y in range(H) for x in range(W))
    assert 0 + R.RH == 6 - 1
    # one row / one column in the last tile, and a last tile that lies wholly inside its neighbour's halo
    assert want[(3, 17, 33)][2:4] == (1, 1) and want[(1, 16, 37)][3] == R.RH and want[(3, 21, 43)][2] == R.RH
    # a partial column tile exists (1920 = 60 * 32 has none), and the content shape has partial tiles both ways
    assert R.CONTENT_SHAPE[1] % R.FH and R.CONTENT_SHAPE[2] % R.FW and R.refine_blocks(*R.CONTENT_SHAPE) == 18


def test_refinement_contents_reach_their_regimes():
    cs = {k: R.refine_case("content " + k) for k in R.CONTENTS}
    for k, c in cs.items():
        assert c["image"].shape == R.CONTENT_SHAPE and c["image"].dtype == F32 and c["gt"].dtype == F32
    w = R.W64
    for k in ("smooth_converged", "flat_offset"):
        x, y = cs[k]["image"].astype(np.float64), cs[k]["gt"].astype(np.float64)
        assert 0 < np.abs(x - y).max() < 5e-3 and y.min() > 0.6                     # near convergence, bright
        mu, s1 = OL._blur(x, w), OL._blur(x * x, w)
        inner = (slice(None), slice(R.RH, -R.RH), slice(R.RH, -R.RH))
        sig = (s1 - mu * mu)[inner]
        # the variance is far below E[x^2] and below C2: E[x^2] - mu^2 cancels in float32, and dm/ds1 ~ -1 / C2 amplifies what is left
        assert sig.max() < 0.03 ** 2 and sig.max() < 1e-3 * s1[inner].min()
        o = R.refine_model(cs[k]["image"], cs[k]["gt"], 1.0)
        assert np.abs(o["partial_blurs"][1][inner]).max() > 500
    assert np.array_equal(cs["flat_equal"]["image"], cs["flat_equal"]["gt"]) and (cs["flat_equal"]["gt"] == F32(0.9)).all()
    assert not cs["black"]["image"].any() and not cs["black"]["gt"].any()
    # l1_ties: exact zeros on both sides of every tile seam and in the four corners, and nowhere else
    t = cs["l1_ties"]
    zero = (t["image"] == t["gt"]).all(axis=0)
    H, W = zero.shape
    pos = R.l1_tie_positions(H, W)
    assert all(zero[y, x] for y, x in pos) and zero.sum() <= len(pos) + 40          # (+ clamped pixels of the noise: 0 == 0, 1 == 1)
    assert all(zero[y, x] for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)))
    assert zero[15].any() and zero[16].any() and zero[31].any() and zero[32].any() and zero[:, 31].any() and zero[:, 32].any()
    assert not (cs["noise"]["image"] == cs["noise"]["gt"]).all(axis=0)[1:-1, 1:31].all()


def test_eval_cases_reach_their_edges():
    for shape in R.EVAL_SHAPES:
        c = R.eval_case(R.shape_name(shape))
        r, g = c["render"], c["gt"]
        assert r.shape == shape and r.dtype == F32 and g.dtype == F32
        if r.size >= len(R.EVAL_SPECIALS):
            assert (r < 0).any() and (r == 0).any() and (r == 1).any() and ((r > 1) & (r < 10)).any() and (r > 1e5).any()
            assert (g == 0).any() and (g == R.TINY).any() and ((g > 0) & (g < R.TINY)).any()
            # the reference's mask counts the subnormal (the fixture decided: test_eval_fixture_against_oracle)
            assert int((g > 0).sum()) == g.size - int((g == 0).sum())
        else:
            assert r.size == 1 and r.item() > 1 and g.item() > 0                    # one pixel, one block: the clamp still acts
    assert [R.eval_case(R.shape_name(s))["edge"]["blocks"] for s in R.EVAL_SHAPES] == [27, 1, 3, 12, 3]
    one = R.eval_case("single element mask")
    assert int((one["gt"] > 0).sum()) == 1 and one["gt"][1, 16, 16] > 0             # alone in the last 1x1 tile
    assert not R.eval_case("empty mask")["gt"].any()
    same = R.eval_case("identical")
    assert np.array_equal(same["render"], same["gt"]) and same["gt"].min() >= 0 and same["gt"].max() <= 1
    cz = R.eval_case("channel zero")["gt"]
    assert (cz[1] == 0).any() and ((cz[1] == 0) & (cz[0] > 0) & (cz[2] > 0)).sum() == (cz[1] == 0).sum()


def test_mapping_cases_reach_their_edges():
    for n in R.MAPPING_HW:
        e = R.mapping_case("hw %d" % n)["edge"]
        assert e["HW"] == n and e["blocks"] == -(-n // 256) and e["tail"] == n % 256
    assert [n % 256 for n in R.MAPPING_HW] == [1, 63, 64, 255, 0, 1, 193] and 63 < 64 < 255 < 256      # below a wave, a wave, a block
    g = R.GRID_STRIDE_HW
    assert -(-g // R.BLOCK) > R.MAX_LOSS_BLOCKS and g - R.MAX_LOSS_BLOCKS * R.BLOCK == 257                 # a ragged second round
    # rgb ties: a pixel exactly on the threshold, one each side, and two whose sum depends on the order
    c = R.mapping_case("rgb ties")
    t = c["gt_image"].reshape(3, -1)
    kinds, thr = c["edge"]["kinds"], R.THR
    left = (t[0] + t[1]) + t[2]
    right = t[0] + (t[1] + t[2])
    assert left.dtype == F32
    k = {name: np.flatnonzero(kinds == i) for i, name in enumerate(R.RGB_TIE_KINDS)}
    assert all(len(v) >= 40 for v in k.values()) and kinds[256] < len(R.RGB_TIE_KINDS)                   # the tail pixel holds one, too
    assert (left[k["exact"]] == thr).all()
    assert (left[k["below"]] == np.nextafter(thr, F32(0))).all() and (left[k["above"]] == np.nextafter(thr, F32(1))).all()
    assert (left[k["left side only"]] > thr).all() and not (right[k["left side only"]] > thr).any()
    assert (right[k["right side only"]] > thr).all() and not (left[k["right side only"]] > thr).any()
    assert np.array_equal(t.sum(axis=0), left)                                                         # numpy sums as the kernel does
    # depth ties
    c = R.mapping_case("depth ties")
    d, kinds = c["gt_depth"].reshape(-1), c["edge"]["kinds"]
    assert (d[kinds == 0] == thr).all() and (d[kinds == 1] == np.nextafter(thr, F32(0))).all() and (d[kinds == 2] == np.nextafter(thr, F32(1))).all()
    assert float(thr) != 0.01 and thr == F32(0.01)
    # exact L1 zeros, masked and live
    c = R.mapping_case("l1 zeros")
    z = c["edge"]["zeros"]
    assert (c["image"].reshape(3, -1)[:, z] == c["gt_image"].reshape(3, -1)[:, z]).all() and z.sum() == 86 and z[255]
    assert (c["depth"].reshape(-1)[z] == c["gt_depth"].reshape(-1)[z]).all()
    assert (c["gt_image"].reshape(3, -1)[:, z].sum(axis=0) > thr).any() and (c["gt_depth"].reshape(-1)[z] > thr).any()
    # saturation: sigmoid in float32, as the kernel and the reference write it
    c = R.mapping_case("marker saturation")
    z, y = c["marker"].reshape(-1), c["kp"].reshape(-1)
    assert {(float(a), float(b)) for a, b in zip(z, y)} == {(float(F32(a)), float(F32(b))) for a in R.LOGITS for b in R.SOFT_TARGETS}
    with np.errstate(over="ignore"):
        s = lambda v: F32(1) / (F32(1) + np.exp(-F32(v)))                           # noqa: E731
        assert s(17.0) == F32(1) and s(16.6) < F32(1) and s(-17.0) > 0
        assert np.isinf(np.exp(F32(89.0))) and np.isfinite(np.exp(F32(88.0))) and s(-89.0) == 0 and s(-1e4) == 0 and s(1e4) == 1
        assert 0 < s(-88.0) < R.TINY                                                # sigmoid(-88) is a subnormal; log of it is -88, not -100
    # every size case holds masked pixels, invalid depths and L1 zeros once it has 16 pixels
    c = R.mapping_case("hw 63")
    assert (c["gt_image"].reshape(3, -1).sum(axis=0) == 0).sum() == 8 and (c["gt_depth"] == 0).sum() == 8
    assert (c["image"] == c["gt_image"]).all(axis=0).sum() >= 4


# ---- every wrong model deviates by more than the bound ---------------------------------------------------------------------------------
# The bounds here are the ones the device tests use, floors included (scalar_bound, map_bound and marker_bound return the larger of
# MARGIN * E_ref and their floor): a model that exceeds them exceeds the floor too, so none is let through by a floor.
@pytest.mark.parametrize("model", list(R.REFINE_WRONG))
def test_refinement_wrong_models_exceed_the_bound(gold, model):
    kw, name, lam, what = R.REFINE_WRONG[model]
    c = R.refine_case(name)
    o = OL.refinement_loss(c["image"], c["gt"], lam)
    bad = R.refine_model(c["image"], c["gt"], lam, **kw)
    if what == "ssim":
        bound = R.scalar_bound(gold[f"refine__{name}__lam{lam}__terms"][1], o["ssim"])
        dev = abs(bad["ssim"] - o["ssim"])
    else:
        bound = R.map_bound(gold[f"refine__{name}__lam{lam}__grad"], o["dL_dimage"])
        dev = np.abs(bad["dL_dimage"] - o["dL_dimage"]).max()
    print(f"{model}: deviation {dev:.3e} = {dev / bound:.1f} x the bound {bound:.3e} on {name}, lambda {lam}")
    assert R.exceeds(dev, bound) and dev > 2 * bound


def test_a_short_halo_hides_under_the_old_tolerance_at_lambda_02(gold):
    """what the suite could not see before: one ring short at every tile seam stays within 3e-4 of the gradient's maximum at lambda 0.2"""
    c = R.refine_case("content noise")
    o = OL.refinement_loss(c["image"], c["gt"], 0.2)
    bad = R.refine_model(c["image"], c["gt"], 0.2, fwd=R.fetch_short_halo(R.FH, R.FW))
    dev = np.abs(bad["dL_dimage"] - o["dL_dimage"]).max()
    assert dev < 3e-3 * np.abs(o["dL_dimage"]).max()
    assert dev > 100 * R.map_bound(gold["refine__content noise__lam0.2__grad"], o["dL_dimage"])


@pytest.mark.parametrize("model", list(R.EVAL_WRONG))
def test_eval_wrong_models_exceed_the_bound(gold, model):
    kw, name, outs = R.EVAL_WRONG[model]
    c = R.eval_case(name)
    o, bad = OL.eval_metrics(c["render"], c["gt"]), R.eval_model(c["render"], c["gt"], **kw)
    ref = dict(zip(("psnr", "ssim", "mse", "count"), gold[f"eval__{name}__out"]))
    for k in outs:
        bound = 0 if k == "count" else R.scalar_bound(ref[k], o[k])
        dev = abs(bad[k] - o[k])
        print(f"{model}: {k} deviates by {dev:.3e}, bound {bound:.3e}")
        assert R.exceeds(dev, bound) and dev > 2 * bound


@pytest.mark.parametrize("model", list(R.MAPPING_WRONG))
def test_mapping_wrong_models_exceed_the_bound(gold, model):
    kw, name, outs = R.MAPPING_WRONG[model]
    c = R.mapping_case(name)
    for ex_name, ex in R.EXPOSURES.items():
        o, bad = _oracle_mapping(c, ex), R.mapping_model(c, ex, **kw)
        pre = f"mapping__{name}__{ex_name}__"
        for k in outs:
            if k == "loss_rgbd":
                assert R.exceeds(abs(bad[k] - o[k]), R.scalar_bound(gold[pre + "loss"][0], o[k])), (model, k)
            elif k == "loss_bce":
                assert R.exceeds(abs(bad[k] - o[k]), R.scalar_bound(gold[pre + "loss"][1], o[k])), (model, k)
            elif k == "dL_dmarker":
                assert R.exceeds(np.abs(bad[k] - o[k]).max(), R.marker_bound(gold[pre + "g_marker"], o[k])), (model, k)
            else:
                ulps = R.ulps_apart(np.asarray(bad[k], F32), np.asarray(o[k], F32)).max()
                assert ulps > {"dL_dimage": R.G_IMAGE_ULPS, "dL_ddepth": R.G_DEPTH_ULPS}[k], (model, k)


# ---- the C ABI's argument checks (before any HIP call) -----------------------------------------------------------------------------------
def _lib():
    from splatloc_amd import _native
    return _native.load()


def test_loss_entry_points_reject_bad_arguments():
    from splatloc_amd import _native
    lib = _lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    thr = C.c_float(0.01)
    views = (_native.LossView * 9)()
    for v in views:
        for f, _ in _native.LossView._fields_:
            setattr(v, f, p.value)
    BAD = 1
    # n_views outside 1 .. 8
    for n in (0, 9, -1):
        assert lib.splatraster_mapping_loss_window(n, 64, views, thr, p, p, None) == BAD, n
    # sizes
    for hw in (0, -5):
        assert lib.splatraster_mapping_loss_window(1, hw, views, thr, p, p, None) == BAD
        assert lib.splatraster_mapping_loss(hw, *([p] * 6), thr, *([p] * 6), None) == BAD
    for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0), (-1, 4, 4), (3, -4, 4), (3, 4, -4)):
        assert lib.splatraster_refinement_loss(*shape, C.c_float(0.2), p, p, p, p, p, None) == BAD, shape
        assert lib.splatraster_eval_metrics(*shape, p, p, p, p, None) == BAD, shape
        assert lib.splatraster_refinement_loss_workspace_bytes(*shape) == 0 and lib.splatraster_eval_metrics_workspace_bytes(*shape) == 0
    assert lib.splatraster_mapping_loss_workspace_bytes(0) == 0 and lib.splatraster_mapping_loss_workspace_bytes(-7) == 0
    # null pointers: every required one, one at a time (exposure, the pointer after kp, may be NULL: that call would launch)
    assert lib.splatraster_mapping_loss_window(1, 64, None, thr, p, p, None) == BAD
    assert lib.splatraster_mapping_loss_window(1, 64, views, thr, None, p, None) == BAD
    assert lib.splatraster_mapping_loss_window(1, 64, views, thr, p, None, None) == BAD
    for f, _ in _native.LossView._fields_:
        if f == "exposure":
            continue
        one = (_native.LossView * 2)()
        for v in one:
            for g, _ in _native.LossView._fields_:
                setattr(v, g, p.value)
        setattr(one[1], f, None)                                                    # the second view's: every view is checked
        assert lib.splatraster_mapping_loss_window(2, 64, one, thr, p, p, None) == BAD, f
    for k in range(12):
        if k == 6:
            continue
        ptrs = [p] * 12
        ptrs[k] = None
        assert lib.splatraster_mapping_loss(64, *ptrs[:6], thr, *ptrs[6:], None) == BAD, k
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert lib.splatraster_refinement_loss(1, 2, 2, C.c_float(0.2), *ptrs, None) == BAD, k
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert lib.splatraster_eval_metrics(1, 2, 2, *ptrs, None) == BAD, k


def test_workspace_sizes_match_the_block_counts():
    lib = _lib()
    align = lambda v: -(-v // 256) * 256                                            # noqa: E731
    for shape in R.REFINE_SHAPES + (R.CONTENT_SHAPE, (3, 1080, 1920)):
        n = shape[0] * shape[1] * shape[2]
        # three float maps (dm/dmu1, dm/ds1, dm/ds12), then two doubles per block: two sections of the workspace walk
        # (csrc/common.h, Carver), each padded to 256 bytes
        assert lib.splatraster_refinement_loss_workspace_bytes(*shape) == \
            align(3 * 4 * n) + align(R.refine_blocks(*shape) * 2 * 8), shape
    for shape in R.EVAL_SHAPES + ((3, 120, 160),):
        assert lib.splatraster_eval_metrics_workspace_bytes(*shape) == R.eval_blocks(*shape) * 3 * 8, shape
    for n in R.MAPPING_HW + (R.GRID_STRIDE_HW,):
        assert lib.splatraster_mapping_loss_workspace_bytes(n) == min(-(-n // R.BLOCK), R.MAX_LOSS_BLOCKS) * 5 * 8, n
