"""The frame-preparation stage on the device (csrc/image_ops.hip, splatloc_amd/image_ops.py) against tests/image_ops_reference.py and
the fixture tests/golden/image_ops.npz (the reference's own image_gradient, image_gradient_mask, Camera.compute_grad_mask and
get_median_depth on the CPU).

Three kinds of check.  Exact and independent of rounding: every returned threshold is edge_threshold times the lower median of the
device's OWN returned intensities over that block or frame, bit for bit, and the 0 / 1 output is the rule applied to those intensities
and thresholds.  Against the fixture: gradients and intensities within four times the reference's own float32 error against the
float64 oracle (taken from the fixture), the 0 / 1 region exact except at pixels the oracle puts within that bound of their threshold
(none, for the seeds of the cases: tests/test_host_image_ops.py asserts it).  Against the float32 restatement in the kernel's stated
summation order: bit for bit, also for the two cases at the LDS path boundary, which are too large for a fixture.  Needs an MI355X."""
import os
import types

import numpy as np
import pytest
import torch

from tests import image_ops_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "image_ops.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def same(a, b):
    """bit for bit (NaN payloads aside)"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def run_case(name):
    from splatloc_amd import image_ops
    c = R.CASES[name]
    img = R.case_image(name)
    out, x, ts = image_ops.compute_grad_masks(torch.from_numpy(img).to(DEV)[None], c["thr"], c["type"], return_intensity=True,
                                              return_thresholds=True)
    assert out.shape == x.shape == (1, 1, c["H"], c["W"]) and x.dtype is torch.float32
    assert out.dtype is (torch.float32 if c["type"] == "replica" else torch.bool)
    assert ts.shape == ((1, 32, 32) if c["type"] == "replica" else (1,))
    return img, out[0, 0].cpu().numpy(), x[0, 0].cpu().numpy(), ts[0].cpu().numpy()


def block_rows(x, bh, bw):
    """the block region of x [H,W] as [1024, bh * bw]: one row per block, blocks row-major"""
    return x[:32 * bh, :32 * bw].reshape(32, bh, 32, bw).transpose(0, 2, 1, 3).reshape(1024, bh * bw)


def check_self_consistent(name, out, x, ts):
    """thresholds and output from the device's own intensities, exactly"""
    c = R.CASES[name]
    H, W = c["H"], c["W"]
    thr = np.float32(c["thr"])
    with np.errstate(invalid="ignore"):
        if c["type"] == "replica":
            bh, bw = H // 32, W // 32
            rows = block_rows(x, bh, bw)
            med = np.sort(rows, axis=1)[:, (bh * bw - 1) // 2]        # NaN sorts last: a row with one has it there, fixed below
            med[np.isnan(rows).any(axis=1)] = np.nan
            t = (med * thr).astype(np.float32)
            assert same(t.reshape(32, 32), ts), name
            tcol = t[:, None]
            want = np.where(np.isnan(tcol), rows, ((rows > tcol) & (tcol < 1)).astype(np.float32))
            assert same(want, block_rows(out, bh, bw)), name
            raw = ~R.block_region(H, W)
            assert same(out[raw], x[raw]), name
        else:
            t = np.float32(R.lower_median(x) * thr)
            assert same(np.asarray(t), np.asarray(ts)), name
            assert same(out, x > t), name


def check_restatement(name, img, out, x, ts):
    """bit for bit the float32 model in the kernel's summation order"""
    c = R.CASES[name]
    m = R.grad_mask_model(img, c["thr"], c["type"], np.float32)
    assert same(x, m["intensity"]), name
    assert same(np.asarray(ts), np.asarray(m["thresholds"], np.float32)), name
    assert same(out, m["out"]), name


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_grad_mask_against_fixture(name, golden):
    from splatloc_amd import image_ops
    c = R.CASES[name]
    H, W = c["H"], c["W"]
    img, out, x, ts = run_case(name)
    check_self_consistent(name, out, x, ts)
    check_restatement(name, img, out, x, ts)
    o64 = R.grad_mask_model(img, c["thr"], c["type"], np.float64)
    bound = R.intensity_bound(golden, name, o64)
    dev = np.abs(x.astype(np.float64) - o64["intensity"])
    print(name, "intensity: max deviation", np.nanmax(dev), "bound", bound)
    assert same(np.isnan(x), np.isnan(o64["intensity"])) and np.nanmax(dev) <= bound
    decided, _ = R.decided_region(name, o64)
    near = R.near_threshold(name, o64, bound)
    assert near.sum() <= R.NEAR_MAX_FRACTION * near.size
    if c["golden"] == "packed":
        ref = R.unpack(golden[f"mask__{name}__out_bits"], (H, W))
        assert decided.all() and same((out != 0)[~near], ref[~near]) and np.isin(out, (0.0, 1.0)).all()
        return
    if c["type"] == "replica":
        ref = golden[f"mask__{name}__out"]
        check = decided & ~near
        assert same(out[check], ref[check])
        assert same(np.isnan(out), np.isnan(ref))
        raw = ~decided
        assert np.nanmax(np.abs(out[raw].astype(np.float64) - o64["intensity"][raw]), initial=0.0) <= bound
    else:
        assert same(out[~near], R.unpack(golden[f"mask__{name}__out"], (H, W))[~near])

    # the drop-ins on the gray image the reference forms
    gray = torch.from_numpy(R.gray_of(img, np.float32)[None].copy()).to(DEV)
    gv, gh = image_ops.image_gradient(gray)
    m32 = R.grad_mask_model(img, c["thr"], c["type"], np.float32)
    for key, got in (("grad_v", gv), ("grad_h", gh)):
        got = got[0].cpu().numpy()
        ref = golden[f"mask__{name}__{key}"]
        b = R.map_bound(ref, o64[key])
        print(name, key, "max deviation", np.nanmax(np.abs(got.astype(np.float64) - o64[key])), "bound", b)
        assert same(np.isnan(got), np.isnan(ref)) and np.nanmax(np.abs(got.astype(np.float64) - o64[key])) <= b
        assert same(got, m32[key]), key
    mv, mh = image_ops.image_gradient_mask(gray)
    assert mv.dtype is torch.bool and mv.shape == gray.shape
    valid = R.unpack(golden[f"mask__{name}__valid"], (H, W))
    assert same(mv[0].cpu().numpy(), valid) and same(mh[0].cpu().numpy(), valid)


@pytest.mark.parametrize("name", ["replica_4096x4096", "replica_3616x4640"])
def test_lds_path_boundary(name):
    """n = 16 384 (the last fused shape) and n = 16 385 (the first that selects over global memory)"""
    from splatloc_amd import image_ops
    c = R.CASES[name]
    assert image_ops.path(c["H"], c["W"]) == c["path"]
    img, out, x, ts = run_case(name)
    check_self_consistent(name, out, x, ts)
    check_restatement(name, img, out, x, ts)
    assert 0.005 < (out != 0).mean() < 0.6


def test_outputs_are_optional_and_paths_agree():
    """without the intensity output the oversized path goes through its workspace; the results are the same"""
    from splatloc_amd import image_ops
    for name in ("replica_75x110", "scenes12_75x110"):
        c = R.CASES[name]
        _, out, x, ts = run_case(name)
        img = torch.from_numpy(R.case_image(name)).to(DEV)[None]
        alone = image_ops.compute_grad_masks(img, c["thr"], c["type"])
        assert isinstance(alone, torch.Tensor) and same(alone[0, 0].cpu().numpy(), out)
        o2, t2 = image_ops.compute_grad_masks(img, c["thr"], c["type"], return_thresholds=True)
        assert same(o2[0, 0].cpu().numpy(), out) and same(t2[0].cpu().numpy(), ts)
    # a thin frame whose blocks (8 x 2 048 pixels) exceed the fused kernel's halo: global path, workspace intensities
    H, W = 256, 65536
    assert image_ops.path(H, W) == "global"
    img = np.ascontiguousarray(np.tile(R.frame(67, 1031, 21), (1, 4, 64))[:, :H, :W])
    t = torch.from_numpy(img).to(DEV)[None]
    out = image_ops.compute_grad_masks(t, 4.0, "replica")[0, 0].cpu().numpy()
    o2, x2, t2 = image_ops.compute_grad_masks(t, 4.0, "replica", return_intensity=True, return_thresholds=True)
    assert same(out, o2[0, 0].cpu().numpy())
    m = R.grad_mask_model(img, 4.0, "replica", np.float32)
    assert same(out, m["out"]) and same(x2[0, 0].cpu().numpy(), m["intensity"]) and same(t2[0].cpu().numpy(), m["thresholds"])


@pytest.mark.parametrize("dataset_type", ["replica", "12scenes"])
def test_three_frames_in_one_call(dataset_type):
    from splatloc_amd import image_ops
    frames = np.stack([R.frame(75, 110, 14), R.frame(75, 110, 24, nan=(40, 70)), R.frame(75, 110, 34, scale=255.0)])
    t = torch.from_numpy(frames).to(DEV)
    together = image_ops.compute_grad_masks(t, 1.5, dataset_type, return_intensity=True, return_thresholds=True)
    assert together[0].shape == (3, 1, 75, 110)
    for i in range(3):
        single = image_ops.compute_grad_masks(t[i:i + 1].contiguous(), 1.5, dataset_type, return_intensity=True, return_thresholds=True)
        for a, b in zip(together, single):
            assert same(a[i].cpu().numpy(), b[0].cpu().numpy()), (i, dataset_type)
        m = R.grad_mask_model(frames[i], 1.5, dataset_type, np.float32)
        assert same(together[0][i, 0].cpu().numpy(), m["out"]), (i, dataset_type)
    assert np.isnan(together[1][1].cpu().numpy()).sum() == 9 and not np.isnan(together[1][0].cpu().numpy()).any()


def test_compute_grad_mask_drop_in():
    from splatloc_amd import image_ops
    img = torch.from_numpy(R.case_image("replica_75x110")).to(DEV)
    for dtype_name, dt in (("replica", torch.float32), ("12scenes", torch.bool)):
        cfg = {"Training": {"edge_threshold": 4}, "Dataset": {"type": dtype_name}}
        cam = types.SimpleNamespace(original_image=img, grad_mask=None)
        ret = image_ops.compute_grad_mask(cam, cfg)
        assert cam.grad_mask is ret and ret.shape == (1, 75, 110) and ret.dtype is dt
        assert torch.equal(image_ops.compute_grad_mask(img, cfg), ret)
        assert torch.equal(ret, image_ops.compute_grad_masks(img[None], 4.0, dtype_name)[0])
    with pytest.raises(ValueError, match="32 x 32"):
        image_ops.compute_grad_masks(img[None, :, :31].contiguous(), 4.0, "replica")
    assert image_ops.compute_grad_masks(img[None, :, :31].contiguous(), 4.0, "12scenes").shape == (1, 1, 31, 110)
    with pytest.raises(ValueError, match="contiguous"):
        image_ops.compute_grad_masks(img[None, :, :, ::2], 4.0, "replica")
    with pytest.raises(ValueError, match="float32"):
        image_ops.compute_grad_masks(img[None].double(), 4.0, "replica")


@pytest.mark.parametrize("name", R.MEDIAN_CASES)
def test_get_median_depth(name, golden):
    from splatloc_amd import image_ops
    c = R.median_case(name)
    args = [None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ("depth", "opacity", "mask")]
    med, std, valid = image_ops.get_median_depth(*args, return_std=True)
    want_med, want_std, want_valid = R.median_model(**c)
    assert med.dim() == 0 and std.dim() == 0 and valid.dtype is torch.bool and valid.shape == c["depth"].shape
    assert same(valid.cpu().numpy(), want_valid)
    assert np.float32(med.item()).tobytes() == np.float32(want_med).tobytes() or (np.isnan(med.item()) and np.isnan(want_med))
    alone = image_ops.get_median_depth(*args)
    assert alone.dim() == 0 and same(alone.cpu().numpy(), med.cpu().numpy())
    if np.isnan(want_std):
        assert np.isnan(std.item())                      # an empty selection (a documented difference) and a single element
    else:
        ref = golden[f"median__{name}__out"]
        assert np.float32(med.item()).tobytes() == ref[0].tobytes()
        print(name, "std deviation", abs(std.item() - want_std), "bound", R.std_bound(ref[1], want_std))
        assert abs(std.item() - want_std) <= R.std_bound(ref[1], want_std)
        assert same(valid.cpu().numpy(), R.unpack(golden[f"median__{name}__valid"], c["depth"].shape))


def test_masked_median():
    from splatloc_amd import image_ops

    def want(v, valid=None):
        return np.array([R.median_model(v[i], mask=None if valid is None else valid[i], positive_only=False)[0] for i in range(len(v))],
                        np.float32)

    v = R.negative_values()                               # two rows, both signs
    t = torch.from_numpy(v).to(DEV)
    assert same(image_ops.masked_median(t).cpu().numpy(), want(v))
    valid = np.random.default_rng(8).uniform(size=v.shape) < 0.5
    valid[1] = v[1] < 0                                   # a row of negative values only
    got = image_ops.masked_median(t, torch.from_numpy(valid).to(DEV)).cpu().numpy()
    assert same(got, want(v, valid)) and got[1] < 0
    valid[0] = False                                      # nothing selected: NaN, the other row unaffected
    got = image_ops.masked_median(t, torch.from_numpy(valid).to(DEV)).cpu().numpy()
    assert np.isnan(got[0]) and same(got, want(v, valid))
    v2 = v.copy()
    v2[0, 17] = np.nan                                    # a selected NaN: NaN; an unselected one: ignored
    valid = np.ones(v.shape, bool)
    assert np.isnan(image_ops.masked_median(torch.from_numpy(v2).to(DEV))[0].item())
    valid[0, 17] = False
    assert same(image_ops.masked_median(torch.from_numpy(v2).to(DEV), torch.from_numpy(valid).to(DEV)).cpu().numpy(), want(v2, valid))
    for name in ("all_equal", "lowest_byte", "highest_byte", "even_count", "odd_count"):
        d = R.median_case(name)["depth"]
        for sign in (1.0, -1.0):
            w = (d * np.float32(sign)).reshape(1, -1)
            assert same(image_ops.masked_median(torch.from_numpy(w).to(DEV)).cpu().numpy(), want(w)), (name, sign)
    # more values than one sweep of the grid covers (512 workgroups x 4 096): the grid-stride loop, three rows at once
    big = (np.random.default_rng(9).standard_normal((3, 2_200_003)) * 100).astype(np.float32)
    assert same(image_ops.masked_median(torch.from_numpy(big).to(DEV)).cpu().numpy(), want(big))


def test_do_recon_leaves_grad_masks():
    from splatloc_amd import image_ops
    from splatloc_amd.scene import DEFAULT_CONFIG, SceneModel, do_recon, synthetic_keyframes
    import copy
    dev = torch.device(DEV)
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["Training"]["mapping_itr_num"] = 1
    pipe = types.SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False)
    for on in (False, True):
        frames, _ = synthetic_keyframes(2, 160, 128, P_truth=4000, seed=2, device=dev)
        do_recon(SceneModel(cfg, dev), frames, pipe, torch.zeros(3, device=dev), cfg, refine_iterations=0, seed=1, grad_masks=on)
        for f in frames:
            if not on:
                assert getattr(f, "grad_mask", None) is None
            else:
                assert f.grad_mask.shape == (1, 128, 160) and f.grad_mask.dtype is torch.float32
                assert torch.equal(f.grad_mask, image_ops.compute_grad_masks(f.original_image[None].contiguous(), 4.0, "replica")[0])
