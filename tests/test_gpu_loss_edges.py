"""The loss stage (csrc/losses.hip) against the float64 oracle (oracle/losses.py) at its tile, mask and saturation edges: every case of
tests/loss_reference.py through the public entry points of splatloc_amd.losses and splatloc_amd.evaluation.  The bounds are functions of
the case (tests/loss_reference.py: MARGIN = 4 times the reference's own float32 error E_ref, recorded in tests/golden/loss_edges.npz);
tests/test_host_loss_edges.py proves on the CPU that every case reaches its edge and that every wrong model exceeds these bounds.
Needs an MI355X.

Measured on an MI355X (device error) / E_ref, the bound being 4: per-pixel maps (the image gradient at lambda 0.2 and 1.0; for the mapping
loss dL/dmarker) and the worst scalar of the case (the largest error / bound over the lambdas / exposure variants), with its error / bound
where the one-ulp floor decided.  The mapping gradients g_image and g_depth are 0 ulp from the reference's elements in every case and
variant (1 ulp from the rounded oracle in the grid-stride case).  The SSIM of the one blur body at its two tile shapes is bit-identical in
every case but shape 1x1x1, where it is 1 ulp apart (the two tiles, 16x16 and 32x16, take their shift from different samples).

    stage    case                     map, lambda 0.2   map, lambda 1.0   worst scalar: error/E_ref  error/bound  (which)
                                     (mapping: g_marker)
    refine   shape 1x1x1                0.553             1.000               1.000                   0.250       ssim()
    refine   shape 1x5x5                0.346             0.490               1.000                   0.250       ssim()
    refine   shape 3x6x6                0.458             0.681               1.000                   0.250       loss lam 0.0
    refine   shape 3x16x32              0.386             0.370               1.000                   0.071       loss lam 0.0
    refine   shape 3x17x33              0.301             0.311               0.549                   0.137       loss lam 0.0
    refine   shape 3x15x31              0.285             0.213               0.203                   0.051       ssim()
    refine   shape 1x16x37              0.379             0.287               0.426                   0.107       loss lam 0.2
    refine   shape 3x21x43              0.422             0.382               0.769                   0.192       loss lam 0.0
    refine   shape 3x1400x1             1.189             1.234               2.117                   0.355       loss lam 1.0
    refine   shape 3x1x2752             1.227             1.614               1.000                   0.250       ssim()
    refine   shape 4x17x33              0.394             0.282               0.581                   0.145       loss lam 0.0
    refine   content noise              0.308             0.266               0.288                   0.072       loss lam 0.0
    refine   content smooth_converged   0.132             0.166               0.396                   0.099       ssim()
    refine   content flat_offset        0.130             0.137               0.122                   0.031       loss lam 0.0
    refine   content flat_equal         0.266             1.434               0.000                   0.005       loss lam 1.0
    refine   content black                  -                 -               0.000                   0.000       ssim()
    refine   content l1_ties            0.400             0.337               1.000                   0.250       ssim()
    eval     shape 3x33x47                  -                 -               1.000                   0.118       mse
    eval     shape 1x1x1                    -                 -               1.000                   0.142       ssim
    eval     shape 3x16x16                  -                 -               1.000                   0.250       mse
    eval     shape 3x17x17                  -                 -               1.000                   0.174       mse
    eval     shape 1x5x40                   -                 -               0.912                   0.228       psnr
    eval     single element mask            -                 -               1.000                   0.250       psnr
    eval     identical                      -                 -               0.000                   0.000       ssim
    eval     empty mask                     -                 -               0.242                   0.061       ssim
    eval     channel zero                   -                 -               1.000                   0.250       ssim
    mapping  hw 1                       0.000                 -               1.000                   0.250       l1 terms zero
    mapping  hw 63                      0.689                 -               6.994                   0.875       d/da ab
    mapping  hw 64                      1.045                 -               1.000                   0.250       l1 terms ab
    mapping  hw 255                     1.000                 -               1.000                   0.250       l1 terms ab
    mapping  hw 256                     0.896                 -               1.000                   0.250       d/da zero
    mapping  hw 257                     0.841                 -               0.823                   0.206       l1 terms zero
    mapping  hw 4801                    0.631                 -               1.000                   0.145       l1 terms ab
    mapping  rgb ties                   0.818                 -               1.000                   0.250       l1 terms zero
    mapping  depth ties                 0.857                 -               1.000                   0.250       l1 terms zero
    mapping  l1 zeros                   0.905                 -               1.000                   0.250       bce zero
    mapping  marker saturation          1.276                 -               1.000                   0.250       d/da ab

flat_equal has no meaningful E_ref (a reference error of 7e-9): its gradient is held to the absolute bound flat_equal_grad_bound and uses
0.032 of it.

Two scalars missed their bound when these tests were first run, and the kernels were changed for it (csrc/losses.hip):
  * content smooth_converged, SSIM mean: 4.11 times E_ref.  Every pixel's SSIM carried a float32 cancellation error of about 1e-4
    (sigma = E[x^2] - mu^2 against C2 = 9e-4).  The SSIM kernels now blur the moments of x - c and y - c, c one value per tile (the
    median of three gt samples), with the zero padding accounted for exactly (SHIFTED MOMENTS in losses.hip): 0.40 times E_ref, and
    flat_offset went from 0.24 to 0.12.  The SSIM partials are formed in double and rounded once: in float32 the roundings of the four
    factors alone put the gradient of shape 1x1x1 one ulp of itself off, over its bound.
  * mapping hw 63, BCE mean: one float32 step from the reference, 1.009 of the one-ulp floor, from logf's one ulp on logarithms that
    reach 8.  The kernel now takes the two logarithms in double: 1.05e-9 from the oracle, the reference's own error, 0.009 of the bound.
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import losses as OL
from tests import loss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden", "loss_edges.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _refine_oracle(name, lam):
    c = R.refine_case(name)
    return OL.refinement_loss(c["image"], c["gt"], lam)


def _report(stage, case, what, dev, e_ref, bound):
    """one line per figure; (device error) / E_ref where E_ref is not 0"""
    ratio = dev / e_ref if e_ref > 0 else float("nan")
    print(f"RATIO {stage} | {case} | {what} | dev {dev:.3e} | E_ref {e_ref:.3e} | ratio {ratio:.3f} | dev/bound {dev / bound if bound > 0 else float('nan'):.3f}")


def _check_scalar(misses, stage, case, what, got, ref32, oracle64, floor=0.0):
    """every figure is printed and every miss is kept: the test asserts once, at its end, that there is none"""
    bound = max(R.scalar_bound(ref32, oracle64), floor)
    dev = abs(float(got) - float(oracle64))
    _report(stage, case, what, dev, abs(float(ref32) - float(oracle64)), bound)
    if not dev <= bound:
        misses.append((case, what, float(got), float(oracle64), f"dev {dev:.4e} > bound {bound:.4e}"))


def _check_refine_grad(misses, name, lam, got, ref32, o, sign=1.0, what="grad"):
    c = R.refine_case(name)
    want = sign * o["dL_dimage"]
    dev = float(np.abs(got.astype(np.float64) - want).max())
    if name == "content black":
        assert not got.any(), (name, lam)                      # exactly 0
        return
    if name == "content flat_equal":
        bound = R.flat_equal_grad_bound(c["image"], c["gt"], lam)
        e_ref = float(np.abs(sign * ref32.astype(np.float64) - want).max())
    else:
        bound = R.map_bound(sign * ref32, want)
        e_ref = float(np.abs(sign * ref32.astype(np.float64) - want).max())
    _report("refine", name, f"{what} lam {lam}", dev, e_ref, bound)
    if not dev <= bound:
        misses.append((name, lam, what, f"dev {dev:.4e} > bound {bound:.4e}"))


# ---- refinement loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.refine_case_names())
def test_refinement_loss_value_terms_and_gradient(gold, name):
    """refinement_loss, refinement_loss_and_grad, ssim and l1_loss: value, both terms and the per-pixel gradient at all three lambdas"""
    from splatloc_amd.losses import _refinement_loss_launch, l1_loss, refinement_loss, refinement_loss_and_grad, ssim
    c = R.refine_case(name)
    gt = _t(c["gt"])
    misses = []
    assert R.refine_blocks(*c["image"].shape) == c["edge"].get("blocks", 18)
    for lam in R.LAMBDAS:
        o = _refine_oracle(name, lam)
        terms = gold[f"refine__{name}__lam{lam}__terms"]
        ref = gold[f"refine__{name}__lam{lam}__grad"]
        x = _t(c["image"], True)
        loss = refinement_loss(x, gt, lam)
        loss.backward()
        g = _np(x.grad)
        _, out = _refinement_loss_launch(x.detach(), gt, lam)
        out = _np(out)
        assert out[2] == float(loss.detach())
        for k, key in enumerate(("l1", "ssim", "loss")):
            _check_scalar(misses, "refine", name, f"{key} lam {lam}", out[k], terms[k], o[key],
                          floor=R.loss_floor(lam, o["l1"], o["ssim"]) if key == "loss" else 0.0)
        if name == "content black":
            assert out[0] == 0 and out[1] == 1.0 and out[2] == 0      # 1 - ssim is exactly 0
        if name == "content flat_equal":
            assert out[0] == 0
        _check_refine_grad(misses, name, lam, g, ref, o)
        value, g2 = refinement_loss_and_grad(_t(c["image"]), gt, lam)
        assert float(value) == out[2] and np.array_equal(_np(g2).view(np.int32), g.view(np.int32))     # the same launch: bit for bit
    # the drop-in functions, as the reference's training loop composes them
    x = _t(c["image"], True)
    s = ssim(x, gt)
    s.backward()
    _check_scalar(misses, "refine", name, "ssim()", float(s.detach()), gold[f"refine__{name}__lam1.0__terms"][1], _refine_oracle(name, 1.0)["ssim"])
    _check_refine_grad(misses, name, 1.0, _np(x.grad), gold[f"refine__{name}__lam1.0__grad"], _refine_oracle(name, 1.0), sign=-1.0, what="d ssim()")
    x = _t(c["image"], True)
    l1 = l1_loss(x, gt)
    l1.backward()
    _check_scalar(misses, "refine", name, "l1_loss()", float(l1.detach()), gold[f"refine__{name}__lam0.0__terms"][0], _refine_oracle(name, 0.0)["l1"])
    _check_refine_grad(misses, name, 0.0, _np(x.grad), gold[f"refine__{name}__lam0.0__grad"], _refine_oracle(name, 0.0), what="d l1_loss()")
    if name == "content l1_ties":
        zero = (c["image"] == c["gt"])
        assert zero.sum() > 100 and not _np(x.grad)[zero].any() and _np(x.grad)[~zero].all()           # sign(0) = 0, exactly
    assert not misses, misses


@pytest.mark.parametrize("name", ["shape 3x17x33", "content smooth_converged"])
def test_refinement_loss_non_contiguous_input_and_upstream_gradient(name):
    """the image as a strided view of a wider tensor, then the ground truth as one, with an upstream gradient of 2.5: the values of the
    contiguous run, and 2.5 times its gradient (one float32 product, as autograd forms it), bit for bit"""
    from splatloc_amd.losses import refinement_loss
    c = R.refine_case(name)
    gt = _t(c["gt"])
    x = _t(c["image"], True)
    loss = refinement_loss(x, gt, 0.2)
    loss.backward()
    want = (torch.tensor(2.5, device=DEV) * x.grad).cpu().numpy()
    C, H, W = c["image"].shape
    wide = torch.full((C, H, 2 * W), 7.0, device=DEV)
    wide[:, :, ::2] = _t(c["image"])
    wide.requires_grad_(True)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    l2 = refinement_loss(view, gt, 0.2)
    assert float(l2.detach()) == float(loss.detach())
    (2.5 * l2).backward()
    got = _np(wide.grad)
    assert np.array_equal(got[:, :, ::2].view(np.int32), want.view(np.int32)) and not got[:, :, 1::2].any()
    gt_wide = torch.zeros((C, 2 * H, W), device=DEV)
    gt_wide[:, 1::2] = gt
    x3 = _t(c["image"], True)
    l3 = refinement_loss(x3, gt_wide[:, 1::2], 0.2)                      # a strided ground truth
    (2.5 * l3).backward()
    assert float(l3.detach()) == float(loss.detach()) and np.array_equal(_np(x3.grad).view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name", [R.shape_name(s) for s in R.REFINE_SHAPES] + ["content noise", "content l1_ties", "content black"])
def test_the_two_blur_bodies_agree(name):
    """one blur body, two tile shapes: eval_metrics_kernel instantiates it on a 16x16 tile with one output per work item, the refinement
    kernels on 32x16 tiles with register-blocked passes; the blurred values do not depend on that, the per-tile shift does: on inputs
    already in [0, 1] the two SSIM means agree to one float32 ulp"""
    from splatloc_amd.evaluation import eval_metrics
    from splatloc_amd.losses import ssim
    c = R.refine_case(name)
    assert c["image"].min() >= 0 and c["image"].max() <= 1
    a = float(eval_metrics(_t(c["image"]), _t(c["gt"])).cpu()[1])
    b = float(ssim(_t(c["image"]), _t(c["gt"])))
    ulps = int(R.ulps_apart(np.array([a], F32), np.array([b], F32))[0])
    print(f"RATIO blur bodies | {name} | eval {a!r} refine {b!r} | {ulps} ulp")
    assert ulps <= 1, (name, a, b)


# ---- eval metrics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.eval_case_names())
def test_eval_metrics_at_the_clamp_and_mask_edges(gold, name):
    from splatloc_amd.evaluation import eval_metrics
    c = R.eval_case(name)
    o = OL.eval_metrics(c["render"], c["gt"])
    psnr, ssim, mse, count = gold[f"eval__{name}__out"]
    out = eval_metrics(_t(c["render"]), _t(c["gt"])).cpu().numpy()
    misses = []
    assert int(out[3]) == o["count"] == int(count)                         # exact: the subnormal counts, zero does not
    _check_scalar(misses, "eval", name, "ssim", out[1], ssim, o["ssim"])
    if name == "empty mask":
        assert np.isnan(out[0]) and np.isnan(out[2]) and out[3] == 0        # the reference's mean over nothing
    elif name == "identical":
        assert np.isposinf(out[0]) and out[2] == 0
    else:
        _check_scalar(misses, "eval", name, "psnr", out[0], psnr, o["psnr"])
        _check_scalar(misses, "eval", name, "mse", out[2], mse, o["mse"])
    if name == "single element mask":
        assert out[3] == 1
    assert not misses, misses


# ---- mapping loss -------------------------------------------------------------------------------------------------------------------
def _launch_mapping(c, ex):
    from splatloc_amd.losses import _mapping_loss_launch
    exposure = None if ex is None else _t(np.array(ex, F32))
    gi, gd, gm, out = _mapping_loss_launch(_t(c["image"]), _t(c["depth"]), _t(c["marker"]), _t(c["gt_image"]), _t(c["gt_depth"]), _t(c["kp"]),
                                           float(R.THR), exposure)
    return _np(gi), _np(gd), _np(gm), _np(out)


@pytest.mark.parametrize("name", R.mapping_case_names())
def test_mapping_loss_elementwise_and_terms(gold, name):
    """the gradients element by element in ulps of the reference's element (tests/loss_reference.py: G_DEPTH_ULPS, G_IMAGE_ULPS and the
    argument for them), exactly 0 wherever the reference's is 0, the three terms and the exposure gradients; with and without the
    exposure pair and at a = b = 0"""
    c = R.mapping_case(name)
    misses = []
    for ex_name, ex in R.EXPOSURES.items():
        o = OL.mapping_loss(*R.mapping_inputs(c), float(R.THR), *(ex if ex is not None else (None, None)))
        pre = f"mapping__{name}__{ex_name}__"
        gi, gd, gm, out = _launch_mapping(c, ex)
        ri, rd, rm = gold[pre + "g_image"], gold[pre + "g_depth"], gold[pre + "g_marker"]
        assert gi.shape == ri.shape and gd.shape == rd.shape and gm.shape == rm.shape
        ui, ud = int(R.ulps_apart(gi, ri).max()), int(R.ulps_apart(gd, rd).max())
        print(f"RATIO mapping | {name} | {ex_name} | g_image {ui} ulp | g_depth {ud} ulp")
        assert ud <= R.G_DEPTH_ULPS and ui <= R.G_IMAGE_ULPS, (name, ex_name, ui, ud)
        assert not gi[ri == 0].any() and not gd[rd == 0].any() and gi[ri != 0].all() and gd[rd != 0].all(), (name, ex_name)
        bound = R.marker_bound(rm, o["dL_dmarker"])
        dev = float(np.abs(gm.astype(np.float64) - o["dL_dmarker"].reshape(gm.shape)).max())
        _report("mapping", name, f"g_marker {ex_name}", dev, float(np.abs(rm.astype(np.float64) - o["dL_dmarker"].reshape(rm.shape)).max()), bound)
        if not dev <= bound:
            misses.append((name, ex_name, "g_marker", f"dev {dev:.4e} > bound {bound:.4e}"))
        _check_scalar(misses, "mapping", name, f"l1 terms {ex_name}", out[0], gold[pre + "loss"][0], o["loss_rgbd"])
        _check_scalar(misses, "mapping", name, f"bce {ex_name}", out[1], gold[pre + "loss"][1], o["loss_bce"])
        if ex is None:
            assert out[2] == 0 and out[3] == 0
        else:
            _check_scalar(misses, "mapping", name, f"d/da {ex_name}", out[2], gold[pre + "g_exposure"][0], o["dL_dexposure_a"])
            _check_scalar(misses, "mapping", name, f"d/db {ex_name}", out[3], gold[pre + "g_exposure"][1], o["dL_dexposure_b"])
    assert not misses, misses


def test_mapping_loss_autograd_entry_on_the_ties():
    """mapping_loss_tensors (the autograd Function) hands the same gradients on, with an upstream gradient other than 1"""
    from splatloc_amd.losses import mapping_loss_tensors
    c = R.mapping_case("rgb ties")
    gi, gd, gm, out = _launch_mapping(c, R.EXPOSURES["ab"])
    image, depth, marker = _t(c["image"], True), _t(c["depth"], True), _t(c["marker"], True)
    a, b = _t(np.array([0.13], F32), True), _t(np.array([-0.04], F32), True)
    loss = mapping_loss_tensors(image, depth, marker, _t(c["gt_image"]), _t(c["gt_depth"]), _t(c["kp"]), float(R.THR), a, b)
    assert float(loss.detach()) == float(F32(out[0]) + F32(out[1]))
    (0.5 * loss).backward()                                                 # a power of two: the products are exact
    assert np.array_equal(_np(image.grad), 0.5 * gi) and np.array_equal(_np(depth.grad), 0.5 * gd) and np.array_equal(_np(marker.grad), 0.5 * gm)
    assert float(a.grad) == 0.5 * out[2] and float(b.grad) == 0.5 * out[3]


def test_mapping_loss_grid_stride_against_oracle():
    """2048 * 256 + 257 pixels: 257 more than the 2048 blocks of the launch hold, so 257 threads of the grid take a second pixel each.
    No fixture (its size): the gradients against the oracle's float64 elements rounded to float32, the terms against the oracle within
    the a-priori rounding bounds of tests/loss_reference.py"""
    c = R.mapping_case("grid stride")
    ex = R.EXPOSURES["ab"]
    assert c["W"] == R.GRID_STRIDE_HW
    o = OL.mapping_loss(*R.mapping_inputs(c), float(R.THR), *ex)
    gi, gd, gm, out = _launch_mapping(c, ex)
    oi, od = o["dL_dimage"].astype(F32).reshape(gi.shape), o["dL_ddepth"].astype(F32).reshape(gd.shape)
    ui, ud = int(R.ulps_apart(gi, oi).max()), int(R.ulps_apart(gd, od).max())
    print(f"RATIO mapping | grid stride | g_image {ui} ulp | g_depth {ud} ulp")
    assert ud <= R.G_DEPTH_ULPS and ui <= R.G_IMAGE_ULPS
    assert not gi[oi == 0].any() and not gd[od == 0].any() and gi[oi != 0].all() and gd[od != 0].all()
    tail = slice(R.MAX_LOSS_BLOCKS * R.BLOCK, None)                         # the ragged second round was written
    assert gi[..., tail].any() and gd[..., tail].any() and gm[..., tail].all()
    dev = float(np.abs(gm.astype(np.float64) - o["dL_dmarker"].reshape(gm.shape)).max())
    bound = R.MARGIN * R.EPS32 / gm.size                                    # MARGIN ulps of s = sigmoid(z) in [0.5, 1), over HW
    print(f"RATIO mapping | grid stride | g_marker dev {dev:.3e} bound {bound:.3e}")
    assert dev <= bound
    for k, (got, want, bound) in enumerate(((out[0], o["loss_rgbd"], R.l1_rounding_bound(c, ex)), (out[1], o["loss_bce"], R.bce_rounding_bound(c["marker"], c["kp"])))):
        bound = max(bound, R.ulp32(want))
        print(f"RATIO mapping | grid stride | term {k} dev {abs(float(got) - want):.3e} bound {bound:.3e}")
        assert abs(float(got) - want) <= bound
    gx = np.abs(o["dL_dimage"]) / float(np.exp(F32(ex[0])))
    for k, (got, want, mag) in enumerate(((out[2], o["dL_dexposure_a"], float((gx * np.abs(c["image"])).sum() * np.exp(ex[0]))),
                                          (out[3], o["dL_dexposure_b"], float(gx.sum())))):
        bound = max(R.MARGIN * R.EPS32 * mag, R.ulp32(want))                # product, expf and the final cast: under MARGIN roundings of the sum of magnitudes
        print(f"RATIO mapping | grid stride | exposure {k} dev {abs(float(got) - want):.3e} bound {bound:.3e}")
        assert abs(float(got) - want) <= bound


@pytest.mark.parametrize("V", [1, 8])
@pytest.mark.parametrize("HW", [255, 257])
def test_window_launch_at_one_and_eight_views(V, HW):
    """mapping_loss_window at the smallest and the largest window and on both sides of one block: bit-identical to the per-view launches"""
    from splatloc_amd.losses import _mapping_loss_launch, mapping_loss_window
    cfg = {"Training": {"rgb_boundary_threshold": float(R.THR)}}
    base = R.mapping_case("hw %d" % HW)
    ties = R.mapping_case("rgb ties")
    rs = np.random.RandomState(V * 1000 + HW)
    for init in (False, True):
        pkgs, vps, single = [], [], []
        for v in range(V):
            render = _t(np.concatenate([rs.rand(3, 1, HW), 8 * rs.rand(1, 1, HW) - 4]).astype(F32))
            depth = _t((3 * rs.rand(1, 1, HW)).astype(F32))
            gt = base["gt_image"].copy() if v % 2 == 0 else rs.rand(3, 1, HW).astype(F32)
            if v == V - 1 and HW == 257:
                gt = ties["gt_image"].copy()                                # threshold ties in a window, too
            gtd = base["gt_depth"].copy() if v % 3 == 0 else (3 * rs.rand(1, HW)).astype(F32)
            vp = types.SimpleNamespace(original_image=_t(gt), depth=gtd if v % 2 else _t(gtd), kp_score=_t((rs.rand(1, HW) ** 4).astype(F32)),
                                       exposure_a=torch.tensor([0.05 * v - 0.1], device=DEV, requires_grad=True),
                                       exposure_b=torch.tensor([0.01 * v], device=DEV, requires_grad=True))
            pkgs.append({"render": render[:3], "depth": depth, "kp_prob": render[-1]})
            vps.append(vp)
            ex = None if init else torch.cat((vp.exposure_a.detach(), vp.exposure_b.detach()))
            single.append(_mapping_loss_launch(pkgs[-1]["render"], depth, pkgs[-1]["kp_prob"], vp.original_image, _t(gtd), vp.kp_score,
                                               float(R.THR), ex))
        tensors, grads, value = mapping_loss_window(cfg, pkgs, vps, initialization=init)
        torch.cuda.synchronize()
        assert len(tensors) == 3 * V and len(grads) == 3 * V
        total = 0.0
        for v in range(V):
            gi, gd, gm, out = single[v]
            for k, want in enumerate((gi, gd, gm)):
                assert torch.equal(grads[3 * v + k].reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)), (v, k)
            total += float(out[0]) + float(out[1])
            if init:
                assert vps[v].exposure_a.grad is None
            else:
                assert float(vps[v].exposure_a.grad) == float(out[2]) and float(vps[v].exposure_b.grad) == float(out[3])
        # value is the float32 sum of the 2 V non-negative terms of the table, in whatever order the reduction takes: 2 V - 1 additions,
        # each rounding by at most half an ulp (EPS32 / 2) of a partial sum that is at most the total, here formed in float64
        assert total > 0 and abs(float(value) - total) <= (2 * V - 1) * 0.5 * R.EPS32 * total
