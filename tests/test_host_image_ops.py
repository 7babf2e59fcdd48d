"""Host-side checks of the frame-preparation stage (include/splatraster.h "frame preparation", csrc/image_ops.hip): the fixture
tests/golden/image_ops.npz (the reference's own functions on the CPU) against the numpy restatement of tests/image_ops_reference.py,
that every case reaches the edge it is named for, that every wrong model is told from the right one, the path hook and the argument
checks of the C ABI (which come before any launch: no device is needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import image_ops_reference as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "image_ops.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def models():
    """name -> (image, float32 model, float64 oracle), computed once"""
    out = {}
    for name in R.GOLDEN_CASES:
        c = R.CASES[name]
        img = R.case_image(name)
        out[name] = (img, R.grad_mask_model(img, c["thr"], c["type"], np.float32), R.grad_mask_model(img, c["thr"], c["type"], np.float64))
    return out


unpack, reference_intensity, intensity_bound = R.unpack, R.reference_intensity, R.intensity_bound


def test_fixture_inputs_are_reproduced(golden):
    for name in R.GOLDEN_CASES:
        assert np.array_equal(golden[f"mask__{name}__checksum"], R.checksum(R.case_image(name))), name
    for name in R.MEDIAN_GOLDEN:
        c = R.median_case(name)
        arrays = [v for v in (c["depth"], c["opacity"], c["mask"]) if v is not None]
        assert np.array_equal(golden[f"median__{name}__checksum"], R.checksum(*arrays)), name


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_fixture_against_restatement(golden, models):
    for name in R.SMALL_CASES:
        c = R.CASES[name]
        img, m32, o64 = models[name]
        shape = (c["H"], c["W"])
        for key in ("grad_v", "grad_h"):
            ref = golden[f"mask__{name}__{key}"]
            bound = R.map_bound(ref, o64[key])
            assert np.isnan(ref).sum() == np.isnan(o64[key]).sum() == np.isnan(m32[key]).sum(), (name, key)
            assert same(np.isnan(ref), np.isnan(m32[key])), (name, key)
            assert np.nanmax(np.abs(m32[key].astype(np.float64) - o64[key])) <= bound, (name, key)
        valid = unpack(golden[f"mask__{name}__valid"], shape)
        assert same(valid, m32["valid"]) and same(valid, o64["valid"]), name
        bound = intensity_bound(golden, name, o64)
        xref = reference_intensity(golden, name, o64)
        assert same(np.isnan(xref), np.isnan(m32["intensity"])), name
        assert np.nanmax(np.abs(m32["intensity"].astype(np.float64) - o64["intensity"])) <= bound, name
        decided, _ = R.decided_region(name, o64)
        if c["type"] == "replica":
            ref = golden[f"mask__{name}__out"]
            assert same(ref[decided], o64["out"][decided].astype(np.float32)) and same(ref[decided], m32["out"][decided]), name
            assert same(np.isnan(ref), np.isnan(m32["out"])), name
            assert np.nanmax(np.abs(m32["out"].astype(np.float64) - o64["out"]), initial=0.0) <= bound, name
        else:
            ref = unpack(golden[f"mask__{name}__out"], shape)
            assert same(ref, o64["out"]) and same(ref, m32["out"]), name
    name = "replica_640x640"
    img, m32, o64 = models[name]
    ref = unpack(golden[f"mask__{name}__out_bits"], (640, 640))
    assert same(ref, o64["out"] != 0) and same(ref, m32["out"] != 0)


def test_no_pixel_is_near_its_threshold(golden, models):
    """the seeds are chosen so that the 0 / 1 decisions of every case are exact: no pixel lies within the bound of its threshold, for the
    reference's own output and therefore for any implementation within the bound"""
    for name in R.GOLDEN_CASES:
        _, _, o64 = models[name]
        near = R.near_threshold(name, o64, intensity_bound(golden, name, o64))
        assert near.sum() == 0, (name, int(near.sum()))
        assert near.sum() <= R.NEAR_MAX_FRACTION * near.size


def test_cases_reach_their_edges(golden, models):
    def n_of(name):
        return (R.CASES[name]["H"] // 32) * (R.CASES[name]["W"] // 32)
    assert n_of("replica_32x32") == 1 and n_of("replica_64x96") == 6 and n_of("replica_96x96") == 9 and n_of("replica_640x640") == 400
    assert n_of("replica_4096x4096") == 16384 and n_of("replica_3616x4640") == 16385
    assert 75 % 32 and 110 % 32                                      # remainder rows and columns
    for name in R.GOLDEN_CASES:
        _, _, o = models[name]
        assert (~o["valid"]).sum() > 0 and o["valid"].sum() > 0, name      # validity matters
        decided, _ = R.decided_region(name, o)
        on = (o["out"] != 0) & decided
        if name == "replica_32x32":
            assert on.sum() == 0          # n = 1: t = 4 x, no pixel exceeds its own threshold
        elif "nan" not in name or R.CASES[name]["type"] == "replica":
            assert 0.004 < on.sum() / decided.sum() < 0.6, (name, on.sum() / decided.sum())     # a mask, neither empty nor full
    # t >= 1: blocks whose threshold is at least 1 hold pixels above it, which the second statement zeroes again
    _, _, o = models["replica_255_64x96"]
    tmap = R.block_thresholds_map(o["thresholds"], 64, 96)
    assert ((tmap >= 1) & (o["intensity"] > tmap)).sum() > 100 and ((tmap >= 1) & (o["out"] != 0)).sum() == 0
    assert ((tmap < 1) & (o["out"] != 0)).sum() > 10          # ... and blocks below 1 keep theirs
    # a zero block: t = 0 and x = 0, where x > t and x >= t part
    _, _, o = models["replica_64x96"]
    assert (o["thresholds"] == 0).sum() >= 4
    # one NaN pixel: nine NaN intensities in four blocks (the pixel sits at a block corner), raw there, decided elsewhere
    _, _, o = models["replica_nan_64x96"]
    assert np.isnan(o["intensity"]).sum() == 9 and np.isnan(o["thresholds"]).sum() == 4
    assert np.isnan(golden["mask__replica_nan_64x96__out"]).sum() == 9
    _, _, o = models["scenes12_nan_64x96"]
    assert np.isnan(o["thresholds"]) and o["out"].sum() == 0
    # medians
    sizes = {n: int(R.median_model(**R.median_case(n))[2].sum()) for n in R.MEDIAN_CASES}
    assert sizes["count_0"] == 0 and sizes["count_1"] == 1 and sizes["even_count"] % 2 == 0 and sizes["odd_count"] % 2 == 1
    d = R.median_case("lowest_byte")["depth"].view(np.uint32)
    assert len(np.unique(d >> 8)) == 1 and len(np.unique(d & 255)) > 100
    d = R.median_case("highest_byte")["depth"].view(np.uint32)
    assert len(np.unique(d & 0xFFFFFF)) == 1 and len(np.unique(d >> 24)) > 10
    assert len(np.unique(R.median_case("all_equal")["depth"])) == 1
    c = R.median_case("depth_300x400")
    v = R.median_model(**c)[2]
    assert 0.1 < v.mean() < 0.5 and (c["depth"] < 0).any() and (c["depth"] == 0).any()
    assert (R.negative_values() < 0).mean() > 0.4


def test_medians_against_restatement(golden):
    for name in R.MEDIAN_GOLDEN:
        c = R.median_case(name)
        med, std, valid = R.median_model(**c)
        ref = golden[f"median__{name}__out"]
        assert same(unpack(golden[f"median__{name}__valid"], c["depth"].shape), valid), name
        assert ref[0].tobytes() == np.float32(med).tobytes(), name
        if np.isnan(std):
            assert np.isnan(ref[1]), name
        else:
            assert abs(float(ref[1]) - std) <= R.std_bound(ref[1], std), name
            assert abs(float(np.float32(std)) - std) <= R.std_bound(ref[1], std), name      # a correctly rounded result passes


def test_wrong_models_are_exposed(golden, models):
    """every wrong model moves an output of at least one case beyond what the tests allow"""
    for wrong, kw in R.WRONG_MASK_MODELS.items():
        exposed = []
        for name in R.SMALL_CASES:
            c = R.CASES[name]
            img, _, o64 = models[name]
            w = R.grad_mask_model(img, c["thr"], c["type"], np.float64, **kw)
            bound = intensity_bound(golden, name, o64)
            decided, _ = R.decided_region(name, o64)
            if c["type"] == "replica":
                ref = golden[f"mask__{name}__out"].astype(np.float64)
                wrong_decision = (ref[decided] != w["out"][decided]).any()
                with np.errstate(invalid="ignore"):
                    wrong_raw = (np.abs(ref[~decided] - w["out"][~decided]) > bound).any()
                if wrong_decision or wrong_raw:
                    exposed.append(name)
            elif (unpack(golden[f"mask__{name}__out"], (c["H"], c["W"])) != w["out"]).any():
                exposed.append(name)
        assert exposed, wrong
    exposed = {"upper median": [], "biased std": []}
    for name in R.MEDIAN_GOLDEN:
        c = R.median_case(name)
        ref = golden[f"median__{name}__out"]
        _, std, _ = R.median_model(**c)
        if ref[0].tobytes() != np.float32(R.median_model(upper=True, **c)[0]).tobytes():
            exposed["upper median"].append(name)
        b = R.median_model(biased=True, **c)[1]
        if not np.isnan(std) and abs(b - float(ref[1])) > R.std_bound(ref[1], std):
            exposed["biased std"].append(name)
    assert "even_count" in exposed["upper median"] and "odd_count" not in exposed["upper median"]
    assert exposed["biased std"]
    # the upper median of a block moves a threshold of the even case
    img, _, o64 = models["replica_64x96"]
    w = R.grad_mask_model(img, 4.0, "replica", np.float64, upper=True)
    assert (w["thresholds"] != o64["thresholds"]).sum() > 500


def test_path_hook():
    from splatloc_amd import _native, image_ops
    lib = _native.load()
    for name, c in R.CASES.items():
        assert image_ops.path(c["H"], c["W"]) == c["path"], name
    assert image_ops.path(1080, 1920) == "lds_small"                # 33 x 60 = 1 980 pixels
    assert image_ops.path(31, 640) == image_ops.path(640, 31) == "none"
    assert image_ops.path(2048, 2048) == "lds_big"                  # n = 4 096 > 2 048
    assert image_ops.path(32, 32 * 851) == "lds_small" and image_ops.path(32, 32 * 852) == "lds_big"      # halo 3 * 854 = 2 562 > 2 560
    assert image_ops.path(224, 65536) == "lds_big" and image_ops.path(256, 65536) == "global"          # n = 16 384, halo 20 500 > 20 480
    assert image_ops.path(288, 65536) == "global" and lib.splatraster_debug_image_ops_path(65537, 64) == 0


def test_argument_checks_come_before_any_launch():
    from splatloc_amd import _native
    lib = _native.load()
    BAD, UNSUPPORTED = 1, _native.ERR_UNSUPPORTED
    fake = C.c_void_p(1 << 12)            # never dereferenced: validation comes first
    nb = C.c_size_t(7)
    REPLICA, GLOBAL = 0, 1

    # workspace queries
    assert lib.splatraster_grad_mask_workspace_bytes(1, 480, 640, REPLICA, 0, C.byref(nb)) == 0 and nb.value == 0      # fused: none
    assert lib.splatraster_grad_mask_workspace_bytes(2, 3616, 4640, REPLICA, 0, C.byref(nb)) == 0 and nb.value >= 2 * 3616 * 4640 * 4
    assert lib.splatraster_grad_mask_workspace_bytes(2, 3616, 4640, REPLICA, 1, C.byref(nb)) == 0 and nb.value == 0
    assert lib.splatraster_grad_mask_workspace_bytes(3, 75, 110, GLOBAL, 0, C.byref(nb)) == 0 and nb.value >= 3 * (4096 + 75 * 110 * 4)
    for bad in ((0, 480, 640, REPLICA), (1, 31, 640, REPLICA), (1, 480, 31, REPLICA), (1, 1, 640, GLOBAL), (1, 480, 640, 2), (-1, 480, 640, GLOBAL),
                (1, 65537, 640, GLOBAL)):
        nb.value = 7
        assert lib.splatraster_grad_mask_workspace_bytes(*bad, 0, C.byref(nb)) == BAD and nb.value == 0, bad
    assert lib.splatraster_grad_mask_workspace_bytes(1, 480, 640, REPLICA, 0, None) == BAD

    def grad_mask(N=1, H=480, W=640, images=fake, thr=4.0, eps=0.01, mode=REPLICA, u8=0, out=fake, intensity=None, thresholds=None, ws=fake,
                  ws_bytes=1 << 40):
        return lib.splatraster_grad_mask(N, H, W, images, thr, eps, mode, u8, out, intensity, thresholds, ws, ws_bytes, None)

    assert grad_mask(H=31) == BAD and grad_mask(W=31) == BAD                 # the reference raises on its empty block
    assert grad_mask(N=0) == BAD and grad_mask(N=-3) == BAD
    assert grad_mask(out=None) == BAD and grad_mask(images=None) == BAD
    assert grad_mask(mode=2) == BAD and grad_mask(eps=-1.0) == BAD and grad_mask(thr=float("nan")) == BAD
    assert grad_mask(u8=1) == UNSUPPORTED                                    # the Replica output carries raw intensities
    assert grad_mask(mode=GLOBAL, H=1) == BAD
    assert lib.splatraster_grad_mask_workspace_bytes(1, 75, 110, GLOBAL, 0, C.byref(nb)) == 0
    assert grad_mask(mode=GLOBAL, H=75, W=110, u8=1, ws_bytes=nb.value - 1) == BAD      # one byte short
    assert grad_mask(mode=GLOBAL, H=75, W=110, u8=1, ws=None) == BAD
    assert lib.splatraster_grad_mask_workspace_bytes(1, 3616, 4640, REPLICA, 0, C.byref(nb)) == 0
    assert grad_mask(H=3616, W=4640, ws_bytes=nb.value - 1) == BAD and grad_mask(H=3616, W=4640, ws=None) == BAD

    def gradient(N=1, Cc=3, H=48, W=64, image=fake, eps=0.01, gv=fake, gh=fake, valid=fake):
        return lib.splatraster_image_gradient(N, Cc, H, W, image, eps, gv, gh, valid, None)

    assert gradient(N=0) == BAD and gradient(Cc=0) == BAD and gradient(H=1) == BAD and gradient(W=1) == BAD
    assert gradient(image=None) == BAD and gradient(gv=None, gh=None, valid=None) == BAD and gradient(eps=float("nan")) == BAD
    assert gradient(N=300, Cc=300) == BAD                                    # more planes than a grid's z extent

    assert lib.splatraster_masked_median_workspace_bytes(2, 1000, C.byref(nb)) == 0 and nb.value >= 2 * 4096
    need = nb.value
    for bad in ((0, 1000), (2, -1), (2, (1 << 31) + 1)):
        nb.value = 7
        assert lib.splatraster_masked_median_workspace_bytes(*bad, C.byref(nb)) == BAD and nb.value == 0, bad
    assert lib.splatraster_masked_median_workspace_bytes(2, 1000, None) == BAD

    def median(N=2, n=1000, values=fake, med=fake, ws=fake, ws_bytes=need):
        return lib.splatraster_masked_median(N, n, values, 1, None, 0.95, None, med, None, None, None, ws, ws_bytes, None)

    assert median(N=0) == BAD and median(n=-1) == BAD and median(values=None) == BAD and median(med=None) == BAD
    assert median(ws=None) == BAD and median(ws_bytes=need - 1) == BAD


def test_python_layer_refuses_before_device_work():
    from splatloc_amd import image_ops
    img = torch.zeros(3, 48, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_ops.image_gradient(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_ops.compute_grad_masks(img[None], 4.0, "replica")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_ops.get_median_depth(img[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_ops.masked_median(img[0])
    with pytest.raises(ValueError):
        image_ops.image_gradient(np.zeros((3, 48, 64), np.float32))
    import inspect
    from splatloc_amd import scene
    assert inspect.signature(scene.do_recon).parameters["grad_masks"].default is False
