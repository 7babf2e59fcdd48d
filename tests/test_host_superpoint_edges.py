"""The edge cases of the SuperPoint head without a GPU (tests/superpoint_reference.py): the models of the device algorithm (NMS on
tiles with a halo, selection through chunks, digit passes, a stepped walk and tiled ranks) equal the contract, each of their
defects changes at least one case, and every builder reaches the edge it names.  tests/test_gpu_superpoint_edges.py runs the
same cases on the device."""
import numpy as np
import pytest
import torch

from tests import superpoint_reference as R


# ---- NMS -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reach():
    """r -> (S, contract N)"""
    return {r: (R.reach_case(r)["S"], R.nms(R.reach_case(r)["S"], r)) for r in R.RADII}


@pytest.fixture(scope="module")
def nms_cases(reach):
    """name -> (S, r, contract N): the reach cases, the negative maps over tile edges and the maps of the first tests"""
    cases = {f"reach_r{r}": (S, r, N) for r, (S, N) in reach.items()}
    for name, (S, r) in R.nms_edge_maps().items():
        cases[name] = (S, r, R.nms(S, r))
    for name, c in R.host_cases().items():
        if "N" not in c:
            S = c["S"] if "S" in c else R.scores(c["semi"])
            cases[name] = (S, c["r"], R.nms(S, c["r"]))
    return cases


def _decisive(N, r):
    return [float(N[b, y, x]) for b, (y, x), _ in R.reach_chains(r)]


def _differing(a, b):
    return sorted((int(i), int(y), int(x)) for i, y, x in torch.nonzero(a != b))


@pytest.mark.parametrize("r", R.RADII)
def test_reach_chains_depend_on_a_pixel_5r_away(r, reach):
    S, N = reach[r]
    assert tuple(S.shape) == (2, 131, 137)
    for b, (y, x), (dy, dx) in R.reach_chains(r):
        hy, hx = y - 5 * r * dy, x - 5 * r * dx
        assert max(abs(hy - y), abs(hx - x)) == 5 * r and S[b, hy, hx] == np.float32(0.95) and float(S[b, y, x]) == pytest.approx(0.86)
        # the head, k = 1 and k = 3 survive; k = 0, 2, 4 (the decisive pixel) and 5 do not
        line = [float(N[b, y - (4 - k) * r * dy, x - (4 - k) * r * dx]) > 0 for k in range(6)]
        assert N[b, hy, hx] == np.float32(0.95) and line == [False, True, False, True, False, False]
    assert _decisive(N, r) == [0.0] * 5
    free = R.reach_case(r, heads=False)["S"]
    Nf = R.nms(free, r)
    assert _decisive(Nf, r) == _decisive(free, r) and min(_decisive(Nf, r)) > 0.85
    # the decisive pixels are the first or the last of a tile at both tile sizes
    for _, (y, x), (dy, dx) in R.reach_chains(r):
        for v, d in ((y, dy), (x, dx)):
            assert d == 0 or v % 64 == (0 if d > 0 else 63)


@pytest.mark.parametrize("r", R.RADII)
def test_tiled_nms_needs_the_whole_5r_halo(r, reach):
    S, N = reach[r]
    tile = R.nms_tile_of(r)
    assert tile == (64 if r <= 4 else 32)
    assert torch.equal(R.nms_tiled(S, r, tile, 5 * r), N)
    decisive = sorted((b, y, x) for b, (y, x), _ in R.reach_chains(r))
    short = _differing(R.nms_tiled(S, r, tile, 5 * r - 1), N)
    print(f"r = {r}: a halo of 5 r - 1 changes {short}")
    assert set(short) >= set(decisive)                                            # one pixel short: every decisive pixel
    assert set(_differing(R.nms_tiled(S, r, tile, 4 * r), N)) >= set(decisive)    # one round short


def test_tiled_nms_is_the_contract_on_every_map(nms_cases):
    for name, (S, r, N) in nms_cases.items():
        assert torch.equal(R.nms_tiled(S, r, R.nms_tile_of(r), 5 * r), N), name
    # the maps of the first tests at every radius and both tile sizes
    for name, c in R.host_cases().items():
        if "S" in c:
            for r in R.RADII:
                for tile in (32, 64):
                    assert torch.equal(R.nms_tiled(c["S"], r, tile, 5 * r), R.nms(c["S"], r)), (name, r, tile)


@pytest.mark.parametrize("wrong", R.NMS_TILED_WRONG)
def test_every_defect_of_the_tiled_nms_is_exposed(wrong, nms_cases):
    exposed = [name for name, (S, r, N) in nms_cases.items() if not torch.equal(R.nms_tiled(S, r, R.nms_tile_of(r), 5 * r, wrong), N)]
    print(wrong, exposed)
    assert exposed, f"no case tells the tiled model's defect {wrong!r} from the contract"
    if wrong in ("panel_zero_pad", "outside_zero"):
        assert {"negative_r3", "negative_r6"} <= set(exposed)           # both instantiations


def test_nms_edge_maps_reach_their_edges():
    maps = R.nms_edge_maps()
    for name in ("negative_r3", "negative_r6"):
        S, r = maps[name]
        assert tuple(S.shape) == (1, 72, 88) and float(S.max()) < 0 and R.nms_tile_of(r) == (64 if r == 3 else 32)
    for name in ("quantised_r2", "quantised_r7"):
        S, r = maps[name]
        assert len(S.unique()) == 4
        for e in (32, 64, 96, 128):                                     # equal neighbours across every tile edge
            assert (S[:, :, e - 1] == S[:, :, e]).any() and (S[:, e - 1, :] == S[:, e, :]).any()
    assert {tuple(S.shape) for S, _ in maps.values()} >= {(1, 1, 1), (1, 1, 200), (1, 200, 1), (3, 5, 7), (1, 64, 64), (1, 65, 65)}


# ---- selection -------------------------------------------------------------------------------------------------------------------

def _select_args(c):
    return c["N"], c["thr"], c["K"], c["border"]


@pytest.fixture(scope="module")
def select_cases():
    """the edge cases, then the cases of the first tests (hand-made N, or N of their score map)"""
    cases = R.select_edge_cases()
    for name, c in R.host_cases().items():
        if "N" not in c:
            S = c["S"] if "S" in c else R.scores(c["semi"])
            c = {"N": R.nms(S, c["r"]), "thr": c["thr"], "K": c["K"], "border": c["border"]}
        cases[name] = c
    return cases


@pytest.fixture(scope="module")
def select_results(select_cases):
    return {name: R.select(*_select_args(c)) for name, c in select_cases.items()}


@pytest.fixture(scope="module")
def traces(select_cases):
    out = {}
    for name, c in select_cases.items():
        out[name] = {}
        R.select_device_model(*_select_args(c), trace=out[name])
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_device_model_of_selection_is_the_contract(select_cases, select_results):
    for name, c in select_cases.items():
        got = R.select_device_model(*_select_args(c))
        assert [t.dtype for t in got] == [t.dtype for t in select_results[name]]
        assert _same(got, select_results[name]), name


@pytest.mark.parametrize("wrong", R.SELECT_MODEL_WRONG)
def test_every_defect_of_the_selection_model_is_exposed(wrong, select_cases, select_results):
    small = [n for n in select_cases if n not in ("largest_k", "many_chunks")]
    exposed = [n for n in small if not _same(R.select_device_model(*_select_args(select_cases[n]), wrong=wrong), select_results[n])]
    print(wrong, exposed)
    assert exposed, f"no case tells the selection model's defect {wrong!r} from the contract"


def test_large_cases_expose_what_only_they_reach(select_cases, select_results):
    """the scan over more than 1024 chunk counts with B = 2, and 64 rank tiles"""
    for name, wrong in (("many_chunks", "offsets_stride"), ("largest_k", "ties_without_tile_offset"), ("largest_k", "sel_carry_dropped")):
        assert not _same(R.select_device_model(*_select_args(select_cases[name]), wrong=wrong), select_results[name]), (name, wrong)


def test_selection_builders_reach_their_edges(select_cases, select_results, traces):
    bits = lambda v: int(np.float32(v).view(np.uint32))
    t = traces["production_k"]
    for b in (0, 1):
        assert (t[b]["n"], t[b]["pick_steps"], t[b]["rank_groups"], t[b]["rank_tiles"]) == (12288, 12, 16, 4)
    N = select_cases["production_k"]["N"]
    assert float(N.min()) > 0 and all(len(N[b].unique()) == 12288 for b in (0, 1))

    # long ties: the cut falls inside the 0.5 class, whose members lie in every step of the walk and in every rank tile
    c, (kp, sc, count, cand) = select_cases["long_ties"], select_results["long_ties"]
    assert sorted(c["N"].unique().tolist()) == [0.125, 0.25, 0.375, 0.5, 0.625]
    for b in (0, 1):
        flat = c["N"][b].flatten()
        n_half = int((flat == 0.5).sum())
        assert traces["long_ties"][b]["T"] == bits(0.5) and 1024 < traces["long_ties"][b]["k"] < n_half
        assert sc[b, 4090:].tolist() == [0.5] * 6 and float(sc[b, 0]) == 0.625
        assert all((flat[i:i + 1024] == 0.5).any() for i in range(0, 12288, 1024))
        first = int((sc[b] == 0.5).nonzero()[0])
        idx = (kp[b, first:, 1] * 128 + kp[b, first:, 0]).long()
        assert (idx[1:] > idx[:-1]).all() and len(idx) > 1024 and first % 1024 != 0   # ascending index across rank tiles
        assert torch.equal(idx, (flat == 0.5).nonzero().flatten()[:len(idx)])

    # shared digits: one bin in the two upper passes, the cut on the wanted low byte
    for name, low in (("shared_digits", None), ("shared_digits_low_00", 0x00), ("shared_digits_low_ff", 0xFF)):
        c = select_cases[name]
        key = c["N"].numpy().view(np.uint32).flatten()
        assert len(np.unique(key)) == 12288 and set(key >> 16) == {0x3F00} and c["K"] >= 1100
        T = traces[name][0]["T"]
        assert T == int(np.sort(key)[::-1][c["K"] - 1]) and traces[name][0]["k"] == 1 and (low is None or T & 255 == low)
        assert traces[name][0]["pick_steps"] == 12 and traces[name][0]["rank_tiles"] == 2

    for K in (1, 256, 257, 1024, 1025):
        a, b = traces[f"k{K}_plus_1"][0], traces[f"k{K}_times_3"][0]
        assert (a["n"], b["n"]) == (K + 1, 3 * K)
        assert a["rank_groups"] == b["rank_groups"] == -(-K // 256) and a["rank_tiles"] == b["rank_tiles"] == -(-K // 1024)
        assert b["pick_steps"] == -(-3 * K // 1024) and a["pick_steps"] == -(-(K + 1) // 1024)

    t = traces["largest_k"][0]
    assert (t["n"], t["pick_steps"], t["rank_groups"], t["rank_tiles"]) == (67584, 66, 256, 64)
    assert select_cases["largest_k"]["K"] == 65535 and len(select_cases["largest_k"]["N"].unique()) < 67584   # equal scores among them

    # ragged: lanes straddle rows, the last chunk is partial, the border leaves 31 x 55 candidates per image
    for name, steps in (("ragged_listed", 0), ("ragged_ranked", 2)):
        c, t = select_cases[name], traces[name]
        H, W = c["N"].shape[1:]
        assert W % 8 != 0 and (H * W) % 2048 not in (0, 2047) and (H * W) % 8 != 0 and c["border"] == 3
        assert all(t[b]["n"] == (H - 6) * (W - 6) == 1705 and t[b]["chunks"] == 2 and t[b]["pick_steps"] == steps for b in (0, 1))
    kp, _, count, _ = select_results["ragged_listed"]
    assert count.tolist() == [1705, 1705] and kp[0, 0].tolist() == [3.0, 3.0] and kp[1, 1704].tolist() == [57.0, 33.0]

    c, t = select_cases["many_chunks"], traces["many_chunks"]
    assert tuple(c["N"].shape) == (2, 1025, 2048) and t[0]["chunks"] == 1025 and t[0]["offset_steps"] == 2
    kp, sc, count, cand = select_results["many_chunks"]
    assert cand.tolist() == [3, 2] and count.tolist() == [3, 2]
    assert kp[0, :3].tolist() == [[5.0, 0.0], [2047.0, 1023.0], [0.0, 1024.0]] and kp[1, :2].tolist() == [[7.0, 512.0], [2047.0, 1024.0]]

    assert select_results["mixed_batch"][3].tolist() == [0, 100, 300, 301, 2400] and select_cases["mixed_batch"]["K"] == 300
    assert select_results["mixed_batch"][2].tolist() == [0, 100, 300, 300, 300]
    N = select_cases["mixed_batch"]["N"]
    for b in range(5):                                                   # one call for the batch is the five calls
        one = R.select(N[b:b + 1], 0.005, 300, 0)
        assert all(torch.equal(x[0], y[b]) for x, y in zip(one, select_results["mixed_batch"]))


# ---- descriptors and scores ------------------------------------------------------------------------------------------------------

def test_dense_shape_crosses_rows_and_images():
    kp = R.pixel_keypoints(3, 72, (3, 38))
    assert tuple(kp.shape) == (3, 2520, 2) and 72 % 16 != 0 and 2520 % 16 != 0
    assert kp[0, 0].tolist() == [0.0, 3.0] and kp[2, -1].tolist() == [71.0, 37.0] and kp[1, 72].tolist() == [0.0, 4.0]
    g = torch.Generator().manual_seed(1)
    coarse = torch.randn(3, 256, 5, 9, generator=g)
    d = R.sample(coarse, kp, torch.full((3,), 2520, dtype=torch.int32))
    assert torch.equal(d.permute(0, 2, 1).reshape(3, 35, 72, 256), R.dense(coarse, (3, 38)))


def test_subpixel_keypoints_cover_the_margin_and_the_grid_lines():
    kp = R.subpixel_keypoints(5, 9)
    assert tuple(kp.shape) == (1, 4096, 2) and len(torch.unique(kp[0], dim=0)) == 4096 and torch.equal(kp * 4, torch.round(kp * 4))
    assert float(kp[..., 0].min()) < -7 and float(kp[..., 0].max()) > 79 and float(kp[..., 1].min()) < -7 and float(kp[..., 1].max()) > 47
    assert (kp != torch.round(kp)).any(-1).float().mean() > 0.9            # off the pixel grid
    fl = R.floors(kp, 5, 9)[0]
    assert set(fl[:, 0].tolist()) >= set(range(-2, 10)) and set(fl[:, 1].tolist()) >= set(range(-2, 5))
    d = R.sample(R.one_hot_coarse(5, 9), kp, torch.full((1,), 4096, dtype=torch.int32))[0]
    taps = (d != 0).sum(0)
    assert set(taps.tolist()) == {0, 1, 2, 4}                               # outside, corner or on a line, edge, inside


def test_far_keypoints_give_zero_columns_in_the_restatement():
    kp, far = R.far_keypoints()
    assert torch.isfinite(kp).all() and far[:16].any() and far[16:].any() and (~far[:16]).any() and (~far[16:]).any()
    g = torch.Generator().manual_seed(2)
    coarse = torch.randn(1, 256, 5, 9, generator=g)
    d = R.sample(coarse, kp, torch.full((1,), 32, dtype=torch.int32))[0]
    assert not d[:, far].any() and d[:, ~far].any(0).all() and not torch.isnan(d).any()
    near = kp.clone()
    near[0, far] = 0.0
    assert torch.equal(R.sample(coarse, near, torch.full((1,), 32, dtype=torch.int32))[0][:, ~far], d[:, ~far])


def test_restatement_ignores_the_scale_of_coarse_and_clamps_count():
    g = torch.Generator().manual_seed(3)
    coarse = torch.randn(2, 256, 5, 9, generator=g)
    kp = R.subpixel_keypoints(5, 9, 17, seed=5).expand(2, -1, -1).contiguous()
    full = torch.full((2,), 17, dtype=torch.int32)
    d = R.sample(coarse, kp, full)
    assert torch.equal(R.sample(coarse * 2.0 ** 40, kp, full), d) and torch.equal(R.sample(coarse * 2.0 ** -20, kp, full), d)
    odd = R.sample(coarse, kp, torch.tensor([-3, 22], dtype=torch.int32))
    assert not odd[0].any() and torch.equal(odd[1], d[1])


def test_score_cases_spread_over_the_decades():
    cases = R.score_edge_cases()
    assert all(tuple(s.shape) == (2, 65, 5, 9) for s in cases.values())
    eq = R.scores(cases["equal_logits"])
    assert len(eq.unique()) == 1 and float(eq[0, 0, 0]) == float(np.float32(1) / np.float32(65))
    wide = R.scores64(cases["wide_logits"])
    assert float(wide.max()) > 0.99 and float(wide.min()) < 1e-45            # near one-hot, tails below float32
    assert float(R.scores64(cases["dustbin_plus_30"]).max()) < 1e-9
    assert float(cases["offset_1e4"][0].min()) > 9990 and float(cases["offset_1e4"][1].max()) < -9990
    for name, semi in cases.items():
        rows = R.decade_errors(R.scores(semi), R.scores(semi), R.scores64(semi))
        assert rows and all(got == ref and got <= bound and bound >= float(np.spacing(np.float32(max(top, 1.5e-45)))) for top, got, ref, bound in rows)
        if name == "wide_logits":
            assert len(rows) > 40 and rows[-1][0] == 1e-46
