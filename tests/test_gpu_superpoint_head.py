"""The device SuperPoint head (splatloc_amd/superpoint.py, csrc/superpoint_head.hip) against tests/superpoint_reference.py.

NMS and selection are comparisons, so they are held bit for bit against the restatement applied to the device's own score map,
read back: no tolerance and no excluded case.  Scores and descriptors are float32 arithmetic and are held against the float64
oracle; the bound is four times the restatement's own maximum error on the same case (the convention of tests/loss_reference.py).

Measured on the MI355X, device error / restatement error (the bound is 4):
  scores        cells_3x4 1.247; 1.000 on cells_5x9, over_a_tile, normal_3x4_b2, two_counts, plateau and the three every_pixel cases
                (the maximum errors coincide with torch's CPU softmax there)
  descriptors   cells_3x4 0.768, cells_5x9 0.743, over_a_tile 0.881, normal_3x4_b2 0.670, two_counts 0.773, plateau 0.862,
                descriptor_edges 0.401, every_pixel_b0 0.691, every_pixel_b4 0.786, chain 0.706, chain_corner 0.859,
                chain_horizontal_edge 0.839, chain_vertical_edge 1.204 (the worst), on a cell (3.5, 3.5) 0.886
"""
import numpy as np
import pytest
import torch

from splatloc_amd import superpoint as SP
from tests import superpoint_reference as R

pytestmark = pytest.mark.gpu

CASES = R.host_cases()          # the tile is asserted below: the builders and the device agree on it
MAP_CASES = sorted(n for n, c in CASES.items() if "N" not in c)
SELECT_CASES = sorted(n for n, c in CASES.items() if "N" in c)
SEMI_CASES = sorted(n for n, c in CASES.items() if "semi" in c)
DESC_CASES = sorted(n for n, c in CASES.items() if "coarse" in c)


def _params(c):
    return {"keypoint_threshold": c["thr"], "max_keypoints": c["K"], "remove_borders": c["border"]}


def _device_map(c):
    """the device's own S of a case (its softmax, or the case's hand-made map)"""
    return SP.score_map(c["semi"].cuda(), 0) if "semi" in c else c["S"].cuda()


def _same_selection(got, want):
    kp, sc, count, cand = got
    assert kp.dtype == sc.dtype == torch.float32 and count.dtype == cand.dtype == torch.int32
    assert torch.equal(cand.cpu(), want["candidates"]) and torch.equal(count.cpu(), want["count"])
    assert torch.equal(kp.cpu(), want["keypoints"]) and torch.equal(sc.cpu(), want["scores"])


def test_the_cases_were_built_for_the_device_tile():
    assert SP.nms_tile() == (64, 64)


@pytest.mark.parametrize("name", MAP_CASES)
def test_nms_and_selection_are_exact(name):
    c = CASES[name]
    S = _device_map(c)
    want = R.head({k: v for k, v in c.items() if k != "semi"} | {"S": S.cpu()})
    N = SP.nms(S, c["r"])
    assert torch.equal(N.cpu(), want["N"])
    _same_selection(SP.select(N, **_params(c)), want)


@pytest.mark.parametrize("name", SELECT_CASES)
def test_selection_on_hand_made_maps(name):
    c = CASES[name]
    _same_selection(SP.select(c["N"].cuda(), **_params(c)), R.head(c))


@pytest.mark.parametrize("radius", (1, 2, 3, 5, 8))
def test_other_radii_take_the_same_rule(radius):
    """radii above 4 run the 32 x 32 tiles; the maps cross their edges and the 64 x 64 ones"""
    g = torch.Generator().manual_seed(radius)
    S = torch.rand(2, 72, 88, generator=g)
    S[1, 30:36, 60:70] = 2.0                                            # a plateau across a tile edge
    assert torch.equal(SP.nms(S.cuda(), radius).cpu(), R.nms(S, radius))


@pytest.mark.parametrize("name", SEMI_CASES)
def test_scores_against_float64(name):
    c = CASES[name]
    want = R.scores64(c["semi"])
    ref = float((R.scores(c["semi"]).double() - want).abs().max())
    got = float((SP.score_map(c["semi"].cuda(), 0).cpu().double() - want).abs().max())
    print(f"{name}: scores device {got:.3g}, restatement {ref:.3g}, ratio {got / ref:.3f}")
    assert ref > 0.0 and got <= 4.0 * ref


@pytest.mark.parametrize("name", DESC_CASES)
def test_descriptors_against_float64(name):
    c = CASES[name]
    ref_out = R.head(c)
    kp, count = ref_out["keypoints"], ref_out["count"]
    want = R.sample64(c["coarse"], kp, count)
    ref = float((ref_out["descriptors"].double() - want).abs().max())
    desc = SP.sample(c["coarse"].cuda(), kp.cuda(), count.cuda())
    assert tuple(desc.shape) == (kp.shape[0], 256, kp.shape[1])
    got = float((desc.cpu().double() - want).abs().max())
    if int(count.max()) == 0:
        assert got == 0.0
        return
    print(f"{name}: descriptors device {got:.3g}, restatement {ref:.3g}, ratio {got / ref:.3f}")
    assert ref > 0.0 and got <= 4.0 * ref
    live = torch.arange(kp.shape[1])[None, :] < count[:, None]
    assert not desc.cpu()[~live[:, None, :].expand_as(desc)].any()     # columns beyond the count


def test_a_keypoint_exactly_on_a_cell_and_a_zero_vector():
    """hand-placed (3.5, 3.5): ix = iy = 0, the descriptor is cell (0, 0)'s unit vector ((31, 23) is cell (3, 2)'s); where every
    neighbour is a zero coarse vector the eps path gives 0"""
    g = torch.Generator().manual_seed(31)
    coarse = torch.randn(1, 256, 3, 4, generator=g)
    coarse[0, :, 1:, :2] = 0.0
    kp = torch.tensor([[[3.5, 3.5], [31.0, 23.0], [9.25, 17.75]]])
    count = torch.full((1,), 3, dtype=torch.int32)
    ij = R.grid_coords(kp, 3, 4)[1][0]
    assert ij[:2].tolist() == [[0.0, 0.0], [3.0, 2.0]] and 0 < float(ij[2, 0]) < 1 < float(ij[2, 1]) < 2
    want = R.sample64(coarse, kp, count)
    ref = float((R.sample(coarse, kp, count).double() - want).abs().max())
    desc = SP.sample(coarse.cuda(), kp.cuda(), count.cuda()).cpu()
    got = float((desc.double() - want).abs().max())
    print(f"on a cell: descriptors device {got:.3g}, restatement {ref:.3g}, ratio {got / ref:.3f}")
    assert ref > 0.0 and got <= 4.0 * ref
    assert desc[0, :, :2].any(0).all() and not desc[0, :, 2].any()        # the eps path: 0 / 1e-12
    one_hot = torch.zeros(1, 256, 3, 4)
    one_hot[0, torch.arange(12), torch.arange(12) // 4, torch.arange(12) % 4] = 1.0
    d = SP.sample(one_hot.cuda(), kp.cuda(), count.cuda()).cpu()
    assert d[0, :, 0].nonzero().flatten().tolist() == [0] and d[0, :, 1].nonzero().flatten().tolist() == [11]


@pytest.mark.parametrize("cells", ((3, 4), (5, 9)))
def test_floors_agree_at_every_pixel(cells):
    """coarse = one unit vector per cell: the non-zero channels of a descriptor name the cells with a non-zero weight, i.e.
    floor(ix), floor(iy) and whether the position sits exactly on a grid line.  They equal the restatement's at every pixel."""
    hc, wc = cells
    n = hc * wc
    coarse = torch.zeros(1, 256, hc, wc)
    coarse[0, torch.arange(n), torch.arange(n) // wc, torch.arange(n) % wc] = 1.0
    got = SP.dense_descriptors(coarse.cuda()).cpu()
    want = R.dense(coarse)
    assert torch.equal(got != 0, want != 0)
    fl = R.floors(torch.tensor([[[0.0, 0.0], [8.0 * wc - 1, 8.0 * hc - 1]]]), hc, wc)[0].tolist()
    assert fl == [[-1.0, -1.0], [wc - 1.0, hc - 1.0]]                    # the zero padding is live at the first pixel


@pytest.mark.parametrize("name", ("cells_3x4", "over_a_tile", "two_counts", "every_pixel_b0"))
def test_detect_is_the_staged_calls(name):
    c = CASES[name]
    semi, coarse = c["semi"].cuda(), c["coarse"].cuda()
    out = SP.detect(semi, coarse, c["r"], **_params(c))
    N = SP.score_map(semi, c["r"])
    kp, sc, count, cand = SP.select(N, **_params(c))
    desc = SP.sample(coarse, kp, count)
    for k, v in (("dense_scores", N), ("keypoints", kp), ("scores", sc), ("count", count), ("candidates", cand), ("descriptors", desc)):
        assert torch.equal(out[k], v), k
    # the dense descriptors at a keypoint's pixel are that keypoint's descriptor; a row range is the slice of the whole
    dense = SP.dense_descriptors(coarse)
    H, W = N.shape[1:]
    assert tuple(dense.shape) == (semi.shape[0], H, W, 256)
    for b in range(semi.shape[0]):
        n = int(count[b])
        x, y = kp[b, :n, 0].long(), kp[b, :n, 1].long()
        assert n > 0 and torch.equal(dense[b, y, x], desc[b, :, :n].T)
    part = SP.dense_descriptors(coarse, rows=(5, H - 2))
    assert torch.equal(part, dense[:, 5:H - 2])
    buf = torch.empty_like(part)
    assert SP.dense_descriptors(coarse, rows=(5, H - 2), out=buf) is buf and torch.equal(buf, part)


def test_postprocess_cuts_to_hlocs_shapes():
    c = CASES["two_counts"]
    semi, coarse = c["semi"].cuda(), c["coarse"].cuda()
    out = SP.detect(semi, coarse, c["r"], **_params(c))
    res = SP.postprocess(semi, coarse, c["r"], **_params(c))
    big = SP.postprocess(semi, coarse, c["r"], **_params(c), original_size=(144, 60))     # 72 x 40 network input
    assert len(res) == 2
    for b, (r, g) in enumerate(zip(res, big)):
        n = int(out["count"][b])
        assert tuple(r["keypoints"].shape) == (n, 2) and tuple(r["scores"].shape) == (n,) and tuple(r["descriptors"].shape) == (256, n)
        assert torch.equal(r["keypoints"], out["keypoints"][b, :n]) and torch.equal(r["descriptors"], out["descriptors"][b, :, :n])
        assert torch.equal(r["dense_scores"], out["dense_scores"][b])
        scale = torch.tensor([144 / 72, 60 / 40], dtype=torch.float32, device="cuda")
        assert torch.equal(g["keypoints"], (r["keypoints"] + 0.5) * scale - 0.5)
    mask = SP.sp_kp_mask(res[0]["dense_scores"])
    assert mask.dtype == torch.bool and torch.equal(mask, out["dense_scores"][0] > 0.005)


def test_inputs_are_checked_before_device_work():
    semi, coarse = torch.zeros(1, 65, 3, 4, device="cuda"), torch.zeros(1, 256, 3, 4, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        SP.score_map(torch.zeros(1, 3, 4, 65, device="cuda").permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="float32"):
        SP.score_map(semi.double())
    with pytest.raises(ValueError):
        SP.detect(semi, torch.zeros(1, 256, 3, 5, device="cuda"))
    with pytest.raises(ValueError):
        SP.nms(torch.zeros(1, 24, 32, device="cuda"), 9)
    with pytest.raises(ValueError):
        SP.select(torch.zeros(1, 24, 32, device="cuda"), max_keypoints=0)
    with pytest.raises(ValueError):
        SP.select(torch.zeros(1, 24, 32, device="cuda"), keypoint_threshold=-1.0)
    with pytest.raises(ValueError):
        SP.dense_descriptors(coarse, rows=(3, 25))


# ---- consumers -------------------------------------------------------------------------------------------------------------------
CAMERA = {"model": "PINHOLE", "width": 64, "height": 48, "params": [40.0, 40.0, 31.5, 23.5]}


def _scene():
    """the synthetic room of tests/test_gpu_localize.py (a copy of its helper): 2000 key Gaussians seen by a 64 x 48 camera"""
    from splatloc_amd.decoder import FeatureDecoder
    from tests import decoder_reference as DR
    from tests.golden.make_golden_matching import FH, FK, FW, look_at, ray_depth, wall_points
    rng = np.random.default_rng(77)
    pts = wall_points(rng, 2000).astype(np.float32)
    marker = rng.uniform(0.004, 0.02, size=(len(pts), 1)).astype(np.float32)
    c2w = look_at(np.array([1.5, 1.2, 1.4]), np.array([5.5, 4.0, 1.2])).astype(np.float32)
    depth = ray_depth(c2w.astype(np.float64), FK, FW, FH).astype(np.float32)
    frame = {"K": FK, "c2w": torch.from_numpy(c2w), "w2c": torch.from_numpy(np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)),
             "depth": torch.from_numpy(depth)}
    cfg = DR.office_0_config()
    cfg["scene"] = {"bound": [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]], "voxel_sdf": 0.06}
    torch.manual_seed(0)
    decoder = DR.trained_scale_(FeatureDecoder(cfg).cuda())
    return {"pts": pts, "marker": marker, "frame": frame, "decoder": decoder, "K": FK, "W": FW, "H": FH}


def test_consumers_take_the_heads_outputs():
    """a postprocess dict goes through Localizer as the query, a dense_scores map through frustum_candidates as kp_mask"""
    from splatloc_amd import localize as L
    from splatloc_amd import matching as M
    sc = _scene()
    assert (sc["W"], sc["H"]) == (64, 48)
    c = R.peaked_case(6, 8, 1, 41)
    query = SP.postprocess(c["semi"].cuda(), c["coarse"].cuda())[0]
    n = query["keypoints"].shape[0]
    assert n >= 5 and tuple(query["dense_scores"].shape) == (48, 64)
    mask = SP.sp_kp_mask(query["dense_scores"])
    frame = dict(sc["frame"], sp_kp_mask=mask)
    host_frame = dict(sc["frame"], sp_kp_mask=mask.cpu().to(torch.int32))
    f = sc["frame"]
    got = M.frustum_candidates(sc["pts"], f["w2c"], sc["K"], 64, 48, marker=sc["marker"], kp_mask=mask, depth=f["depth"], c2w=f["c2w"],
                               kp_K=sc["K"])
    want = M.frustum_candidates(sc["pts"], f["w2c"], sc["K"], 64, 48, marker=sc["marker"], kp_mask=mask.cpu().to(torch.int32),
                                depth=f["depth"], c2w=f["c2w"], kp_K=sc["K"])
    assert got[0].numel() > 0 and all(torch.equal(a, b) for a, b in zip(got, want))
    loc = L.Localizer(sc["pts"], sc["marker"], sc["decoder"], sc["K"], sc["W"], sc["H"], CAMERA)
    res = loc.localize([query], [frame], [0])
    host_query = {"keypoints": query["keypoints"].cpu().numpy(), "descriptors": query["descriptors"].cpu().numpy()}
    ref = loc.localize([host_query], [host_frame], [0])
    assert tuple(res["R_c2w"].shape) == (1, 3, 3) and res["success"].dtype == torch.bool
    for k in res:
        assert torch.equal(res[k], ref[k]), k
