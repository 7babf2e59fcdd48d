"""The device SuperPoint head (splatloc_amd/superpoint.py, csrc/superpoint_head.hip) at the edges of its kernels: the whole 5 r
halo of the NMS at every radius, the carries, groups, tiles and digits of the selection at n > K up to K = 65535, compaction over
ragged rows and more than 1024 chunks, the dense descriptors at every pixel across row and image ends, keypoints off the pixel
grid and far outside the image, and scores held per decade.  tests/test_host_superpoint_edges.py shows without a GPU that these
cases reach those edges and that a model of the device algorithm with a defect there fails at least one of them.

NMS and selection are held bit for bit against the restatement (tests/superpoint_reference.py), no tolerance and no excluded
element.  Descriptors and scores are held against the float64 oracle within four times the restatement's own maximum error on
the same case; scores per decade of the expected score, the bound floored at one float32 ulp of the decade's top.

Measured on the MI355X in one run of this file, device error / restatement error (the bound is 4):
  descriptors   dense 3 x 35 x 72 0.694, 4096 sub-pixel keypoints 0.891, neighbours of far keypoints 0.990, K = 17 0.828
  scores        wide_logits (47 bands, 1 down to below 1e-46) 1.000 in 42 of them, 0.975 to 0.982 in three, 1.133 below 1e-45
                (subnormal scores) and 1.000 in the last band; equal_logits 1.000 (bit-equal); dustbin_plus_30 (bands 1e-11 to
                1e-14) 1.000, 1.015, 1.000, 1.000; offset_1e4 (bands 1 to 1e-3) 1.000, 1.266 (the worst), 1.083, 1.000
"""
import ctypes as C

import numpy as np
import pytest
import torch

from splatloc_amd import _native
from splatloc_amd import superpoint as SP
from tests import superpoint_reference as R
from tests.test_gpu_superpoint_head import _same_selection

pytestmark = pytest.mark.gpu

NMS_MAPS = R.nms_edge_maps()
SELECT_CASES = R.select_edge_cases()
SCORE_CASES = R.score_edge_cases()


def _params(c):
    return {"keypoint_threshold": c["thr"], "max_keypoints": c["K"], "remove_borders": c["border"]}


def _want(c):
    return dict(zip(("keypoints", "scores", "count", "candidates"), R.select(c["N"], c["thr"], c["K"], c["border"])))


def _bound(name, got, want, ref):
    """the project's bound: the device's maximum error within four times the restatement's on the same case"""
    e_got, e_ref = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
    print(f"{name}: device {e_got:.3g}, restatement {e_ref:.3g}, ratio {e_got / e_ref:.3f}")
    assert e_ref > 0.0 and e_got <= 4.0 * e_ref


# ---- NMS -------------------------------------------------------------------------------------------------------------------------

def test_the_cases_were_built_for_the_device_tiles():
    assert SP.nms_tile() == (R.EDGE, R.EDGE) and R.nms_tile_of(4) == 64 and R.nms_tile_of(5) == 32


@pytest.mark.parametrize("r", R.RADII)
def test_nms_reaches_5r(r):
    """the decisive pixels lose to a head exactly 5 r away, across a tile edge from either side, along rows, columns and the
    diagonal; without the heads they survive"""
    for heads in (True, False):
        S = R.reach_case(r, heads)["S"]
        N = SP.nms(S.cuda(), r).cpu()
        assert torch.equal(N, R.nms(S, r))
        for b, (y, x), _ in R.reach_chains(r):
            assert (float(N[b, y, x]) == 0.0) == heads


@pytest.mark.parametrize("name", sorted(NMS_MAPS))
def test_nms_on_negative_quantised_and_degenerate_maps(name):
    S, r = NMS_MAPS[name]
    assert torch.equal(SP.nms(S.cuda(), r).cpu(), R.nms(S, r))


# ---- selection -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_selection_at_the_edges_of_its_kernels(name):
    c = SELECT_CASES[name]
    _same_selection(SP.select(c["N"].cuda(), **_params(c)), _want(c))


def test_a_batch_is_its_images_one_by_one():
    c = SELECT_CASES["mixed_batch"]
    N = c["N"].cuda()
    whole = SP.select(N, **_params(c))
    assert whole[3].tolist() == [0, 100, 300, 301, 2400]
    for b in range(N.shape[0]):
        one = SP.select(N[b:b + 1].contiguous(), **_params(c))
        assert all(torch.equal(x[0], y[b]) for x, y in zip(one, whole))


@pytest.mark.parametrize("name", ("long_ties", "mixed_batch", "ragged_ranked"))
def test_selection_ignores_what_the_workspace_held(name):
    c = SELECT_CASES[name]
    N = c["N"].cuda()
    b, h, w = N.shape
    nb = C.c_size_t(0)
    _native.check(_native.load().splatraster_sp_workspace_bytes(b, h, w, c["K"], C.byref(nb)), "splatraster_sp_workspace_bytes")
    want = _want(c)
    for fill in (0xFF, 0x00):
        ws = torch.full((nb.value,), fill, dtype=torch.uint8, device="cuda")
        _same_selection(SP._select(N, float(c["thr"]), c["K"], c["border"], ws), want)


# ---- descriptors -----------------------------------------------------------------------------------------------------------------

def test_dense_descriptors_are_sample_at_every_pixel():
    """W = 72: a wave's 16 pixels cross row ends; 35 rows of 72 are 2520 pixels per image, no multiple of 16: runs cross images"""
    g = torch.Generator().manual_seed(107)
    coarse = torch.randn(3, 256, 5, 9, generator=g)
    rows = (3, 38)
    kp = R.pixel_keypoints(3, 72, rows)
    count = torch.full((3,), kp.shape[1], dtype=torch.int32)
    dense = SP.dense_descriptors(coarse.cuda(), rows=rows).cpu()
    assert tuple(dense.shape) == (3, 35, 72, 256)
    sparse = SP.sample(coarse.cuda(), kp.cuda(), count.cuda()).cpu()
    assert torch.equal(dense, sparse.permute(0, 2, 1).reshape(3, 35, 72, 256))
    _bound("dense 3 x 35 x 72", dense, R.dense(coarse.double(), rows), R.dense(coarse, rows))


def test_subpixel_keypoints_take_the_same_cells_and_the_bound():
    kp = R.subpixel_keypoints(5, 9)
    count = torch.full((1,), kp.shape[1], dtype=torch.int32)
    one_hot = R.one_hot_coarse(5, 9)
    got = SP.sample(one_hot.cuda(), kp.cuda(), count.cuda()).cpu()
    assert torch.equal(got != 0, R.sample(one_hot, kp, count) != 0)         # floors and on-grid-line weights off the pixel grid
    g = torch.Generator().manual_seed(109)
    coarse = torch.randn(1, 256, 5, 9, generator=g)
    got = SP.sample(coarse.cuda(), kp.cuda(), count.cuda()).cpu()
    _bound("4096 sub-pixel keypoints", got, R.sample64(coarse, kp, count), R.sample(coarse, kp, count))


def test_far_keypoints_give_zero_columns():
    kp, far = R.far_keypoints()
    count = torch.full((1,), 32, dtype=torch.int32)
    g = torch.Generator().manual_seed(113)
    coarse = torch.randn(1, 256, 5, 9, generator=g)
    got = SP.sample(coarse.cuda(), kp.cuda(), count.cuda()).cpu()[0]
    assert not got[:, far].any() and not R.sample(coarse, kp, count)[0][:, far].any()
    near = kp.clone()
    near[0, far] = 0.0                                                      # the neighbours in the same 16-keypoint groups
    alone = SP.sample(coarse.cuda(), near.cuda(), count.cuda()).cpu()[0]
    assert got[:, ~far].any(0).all() and torch.equal(got[:, ~far], alone[:, ~far])
    _bound("neighbours of far keypoints", got[:, ~far], R.sample64(coarse, kp, count)[0][:, ~far], R.sample(coarse, kp, count)[0][:, ~far])


def test_count_is_clamped_and_k_need_not_be_a_multiple_of_16():
    g = torch.Generator().manual_seed(127)
    coarse = torch.randn(2, 256, 5, 9, generator=g)
    kp = (R.subpixel_keypoints(5, 9, 17, seed=5) * 0.5 + 20.0).expand(2, -1, -1).contiguous()     # inside the grid of cells
    full = torch.full((2,), 17, dtype=torch.int32)
    d = SP.sample(coarse.cuda(), kp.cuda(), full.cuda()).cpu()
    assert tuple(d.shape) == (2, 256, 17) and d.any(1).all() and R.sample(coarse, kp, full).any(1).all()
    _bound("K = 17", d, R.sample64(coarse, kp, full), R.sample(coarse, kp, full))
    odd = SP.sample(coarse.cuda(), kp.cuda(), torch.tensor([-3, 22], dtype=torch.int32).cuda()).cpu()
    assert not odd[0].any() and torch.equal(odd[1], d[1])                   # -3 as 0, K + 5 as K
    part = SP.sample(coarse.cuda(), kp.cuda(), torch.tensor([16, 1], dtype=torch.int32).cuda()).cpu()
    assert torch.equal(part[0, :, :16], d[0, :, :16]) and not part[0, :, 16].any()
    assert torch.equal(part[1, :, :1], d[1, :, :1]) and not part[1, :, 1:].any()


def test_descriptors_ignore_the_scale_of_coarse():
    g = torch.Generator().manual_seed(131)
    coarse = torch.randn(2, 256, 5, 9, generator=g)
    kp = R.subpixel_keypoints(5, 9, 64, seed=7).expand(2, -1, -1).contiguous()
    count = torch.full((2,), 64, dtype=torch.int32)
    d = SP.sample(coarse.cuda(), kp.cuda(), count.cuda())
    dense = SP.dense_descriptors(coarse.cuda(), rows=(0, 9))
    for scale in (2.0 ** 40, 2.0 ** -20):
        assert torch.equal(SP.sample((coarse * scale).cuda(), kp.cuda(), count.cuda()), d)
        assert torch.equal(SP.dense_descriptors((coarse * scale).cuda(), rows=(0, 9)), dense)


# ---- scores ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_scores_per_decade(name):
    semi = SCORE_CASES[name]
    got, ref, want = SP.score_map(semi.cuda(), 0).cpu(), R.scores(semi), R.scores64(semi)
    rows = R.decade_errors(got, ref, want)
    for top, e_got, e_ref, bound in rows:
        ratio = e_got / e_ref if e_ref > 0 else float("inf") if e_got > 0 else 0.0
        print(f"{name}: scores below {top:.0e}: device {e_got:.3g}, restatement {e_ref:.3g}, ratio {ratio:.3f}, bound {bound:.3g}")
    assert rows and all(e_got <= bound for _, e_got, _, bound in rows)
    if name == "equal_logits":
        assert torch.equal(got, ref) and float(got[0, 0, 0]) == float(np.float32(1) / np.float32(65))
