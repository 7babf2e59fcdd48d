"""The SuperPoint head without a GPU: the CPU restatement (tests/superpoint_reference.py) reaches the edges its cases name, every
wrong model changes the output of at least one case, the float64 oracle sees a non-zero error of the float32 restatement (the GPU
tests' bounds are multiples of it), and the C ABI checks its arguments before any launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import superpoint_reference as R


@pytest.fixture(scope="module")
def cases():
    return R.host_cases()


@pytest.fixture(scope="module")
def results(cases):
    return {name: R.head(c) for name, c in cases.items()}


def _cols(out, b=0):
    n = int(out["count"][b])
    return [int(x) for x in out["keypoints"][b, :n, 0]]


def test_contract_numbers_of_the_grid_rule():
    """the four keypoints the contract lists for Hc x Wc = 3 x 4"""
    kp = torch.tensor([[[4.0, 4.0], [0.0, 0.0], [27.0, 19.0], [31.0, 23.0], [3.5, 3.5]]])
    _, ij = R.grid_coords(kp, 3, 4)
    assert abs(float(ij[0, 0, 0]) - 0.0545) < 5e-5 and abs(float(ij[0, 1, 0]) + 0.3818) < 5e-5 and abs(float(ij[0, 2, 0]) - 2.5636) < 5e-5
    assert ij[0, 3].tolist() == [3.0, 2.0] and ij[0, 4].tolist() == [0.0, 0.0]
    assert R.floors(kp, 3, 4)[0, 1].tolist() == [-1.0, -1.0]          # the zero padding is live at (0, 0)


def test_chain_counts_the_rounds(cases):
    """maxima 3 px apart, descending from column 1: 0 / 1 / 2 / 3 extra rounds keep the first 1 / 2 / 3 / 4 at columns 1, 7, 13, 19"""
    c = cases["chain"]
    assert tuple(c["S"].shape) == (1, 24, 32) and c["r"] == 4
    for wrong, want in (("rounds_0", [1]), ("rounds_1", [1, 7]), (None, [1, 7, 13]), ("rounds_3", [1, 7, 13, 19])):
        assert _cols(R.head(c, wrong)) == want, wrong
    tile = R.tile_chain_cases(64, 64)
    v, h, k = (R.head(tile[n]) for n in ("chain_vertical_edge", "chain_horizontal_edge", "chain_corner"))
    assert _cols(v) == [53, 59, 65] and [int(y) for y in h["keypoints"][0, :3, 1]] == [53, 59, 65] and int(h["count"][0]) == 3
    assert _cols(k) == [58, 64, 70]
    # the corner chain's last maximum sits in the image corner and the clipped window reaches it
    S = tile["chain_corner"]["S"]
    assert float(S[0, -1, -1]) > 0.5 and int(R.head(tile["chain_corner"], "rounds_3")["count"][0]) == 4


def test_cases_reach_their_edges(cases, results):
    assert cases["cells_3x4"]["semi"].shape[2:] == (3, 4)            # 24 x 32 px: smaller than the 20-pixel reach on either side
    assert cases["over_a_tile"]["semi"].shape[2:] == (9, 9)          # one cell over a 64 x 64 tile in each direction
    n = results["over_a_tile"]["candidates"][0]
    assert n > cases["over_a_tile"]["K"]                             # the top-k path with real scores
    # plateau: all 64 pixels of the cell survive with one score
    p = results["plateau"]
    cell = p["N"][0, 16:24, 32:40]
    assert (cell > 0).all() and len(cell.unique()) == 1
    # B = 2 with different counts, one of them cut by K
    t = results["two_counts"]
    assert t["candidates"][0] > cases["two_counts"]["K"] > t["candidates"][1] > 0
    assert t["count"].tolist() == [cases["two_counts"]["K"], int(t["candidates"][1])]
    # threshold: of nextafter-below, equal, nextafter-above only the last is a candidate
    assert _cols(results["threshold"]) == [25]
    # n = K keeps the row-major order, n = K + 1 switches to descending scores
    a, b = results["count_K"], results["count_K_plus_1"]
    assert int(a["candidates"][0]) == 12 == int(a["count"][0]) and int(b["candidates"][0]) == 13 and int(b["count"][0]) == 12
    idx = a["keypoints"][0, :, 1] * 32 + a["keypoints"][0, :, 0]
    assert (idx[1:] > idx[:-1]).all() and not (a["scores"][0, 1:] <= a["scores"][0, :-1]).all()
    assert (b["scores"][0, 1:] < b["scores"][0, :-1]).all()
    # ties: four distinct scores, then the six equal ones with the smallest row-major index
    t = results["ties"]
    assert int(t["candidates"][0]) == 13 and t["scores"][0, 4:].tolist() == [0.25] * 6
    assert [int(y) for y in t["keypoints"][0, 4:, 1]] == [2, 4, 6, 8, 10, 12]
    # none, every pixel, and a border that leaves nothing
    assert int(results["none"]["count"][0]) == 0 and not results["none"]["keypoints"].any()
    e0, e4, e12 = (results[f"every_pixel_b{b}"] for b in (0, 4, 12))
    assert int(e0["candidates"][0]) == 24 * 32 and int(e4["candidates"][0]) == 16 * 24 and int(e12["candidates"][0]) == 0
    assert int(e0["count"][0]) == 64 and (e0["scores"][0, 1:] <= e0["scores"][0, :-1]).all()
    # descriptor edges: border 0 puts (0, 0) and (W - 1, H - 1) among the keypoints
    d = results["descriptor_edges"]
    assert d["keypoints"][0, :4].tolist() == [[0.0, 0.0], [3.0, 3.0], [4.0, 4.0], [31.0, 23.0]]
    fl = R.floors(d["keypoints"][:, :4], 3, 4)[0].tolist()
    assert fl == [[-1.0, -1.0], [-1.0, -1.0], [0.0, 0.0], [3.0, 2.0]]
    assert not d["descriptors"][0, :, 4:].any()


def test_every_wrong_model_is_exposed(cases, results):
    for wrong in R.WRONG:
        exposed = [name for name, c in cases.items() if not R.same(R.head(c, wrong), results[name])]
        assert exposed, f"no case tells the wrong model {wrong!r} from the contract"


def test_float32_restatement_has_an_error_the_bounds_can_rest_on(cases):
    g = torch.Generator().manual_seed(0)
    semi = torch.randn(2, 65, 3, 4, generator=g)
    err = float((R.scores(semi).double() - R.scores64(semi)).abs().max())
    print(f"softmax: max |f32 - f64| = {err:.3g}")
    assert 0.0 < err < 1e-6
    for name in ("cells_3x4", "cells_5x9", "normal_3x4_b2", "descriptor_edges"):
        c, out = cases[name], R.head(cases[name])
        err = float((out["descriptors"].double() - R.sample64(c["coarse"], out["keypoints"], out["count"])).abs().max())
        print(f"{name}: descriptors max |f32 - f64| = {err:.3g}")
        assert 0.0 < err < 1e-5
    # a zero coarse vector takes the eps path and stays zero
    coarse = torch.zeros(1, 256, 3, 4)
    kp = torch.tensor([[[5.0, 7.0]]])
    assert not R.sample(coarse, kp, torch.ones(1, dtype=torch.int32)).any()


def test_dense_restatement_is_sample_at_every_pixel(cases):
    c = cases["cells_3x4"]
    d = R.dense(c["coarse"])
    kp = torch.tensor([[[4.0, 4.0], [31.0, 23.0], [0.0, 0.0]]])
    s = R.sample(c["coarse"], kp, torch.full((1,), 3, dtype=torch.int32))
    assert torch.equal(d[0, 4, 4], s[0, :, 0]) and torch.equal(d[0, 23, 31], s[0, :, 1]) and torch.equal(d[0, 0, 0], s[0, :, 2])
    assert torch.equal(R.dense(c["coarse"], (5, 9)), d[:, 5:9])


def test_argument_checks_come_before_any_launch():
    from splatloc_amd import _native
    lib = _native.load()
    BAD, UNSUPPORTED = 1, _native.ERR_UNSUPPORTED
    fake = C.c_void_p(1 << 12)            # never dereferenced: validation comes first
    odd = C.c_void_p((1 << 12) + 4)
    nb = C.c_size_t(7)
    th, tw = C.c_int32(0), C.c_int32(0)
    assert lib.splatraster_sp_nms_tile(C.byref(th), C.byref(tw)) == 0 and th.value >= 8 and tw.value >= 8
    assert th.value % 8 == 0 and tw.value % 8 == 0
    assert lib.splatraster_sp_nms_tile(None, C.byref(tw)) == BAD and lib.splatraster_sp_nms_tile(C.byref(th), None) == BAD

    assert lib.splatraster_sp_workspace_bytes(2, 480, 640, 4096, C.byref(nb)) == 0
    need = nb.value
    assert need >= 2 * (60 * 80 * 256 * 4 + 480 * 640 * 8 + 4096 * 8)
    for bad in ((0, 480, 640, 4096), (1, 0, 640, 4096), (1, 480, 0, 4096), (1, 480, 640, 0), (1, 480, 640, 65536), (-1, 480, 640, 1)):
        nb.value = 7
        assert lib.splatraster_sp_workspace_bytes(*bad, C.byref(nb)) == BAD and nb.value == 0, bad
    assert lib.splatraster_sp_workspace_bytes(1, 480, 640, 4096, None) == BAD
    assert lib.splatraster_sp_workspace_bytes(1, 1 << 16, 1 << 15, 1, C.byref(nb)) == UNSUPPORTED     # B H W = 2^31
    assert lib.splatraster_sp_workspace_bytes(2, 1 << 15, 1 << 15, 1, C.byref(nb)) == UNSUPPORTED
    assert lib.splatraster_sp_workspace_bytes(1, (1 << 16) - 8, 1 << 15, 1, C.byref(nb)) == 0

    def scores(B=1, Hc=60, Wc=80, semi=fake, out=fake):
        return lib.splatraster_sp_scores(B, Hc, Wc, semi, out, None)

    assert scores(B=0) == BAD and scores(Hc=0) == BAD and scores(Wc=-1) == BAD and scores(semi=None) == BAD and scores(out=None) == BAD
    assert scores(out=odd) == BAD                                        # float4 stores
    assert scores(Hc=1 << 13, Wc=1 << 12) == UNSUPPORTED                 # 2^31 pixels
    assert scores(B=2, Hc=1 << 12, Wc=1 << 12) == UNSUPPORTED

    def nms(B=1, H=480, W=640, s=fake, r=4, out=C.c_void_p(1 << 13)):
        return lib.splatraster_sp_nms(B, H, W, s, r, out, None)

    assert nms(B=0) == BAD and nms(H=0) == BAD and nms(W=0) == BAD and nms(s=None) == BAD and nms(out=None) == BAD
    assert nms(r=-1) == BAD and nms(r=9) == BAD and nms(out=fake) == BAD and nms(H=1 << 16, W=1 << 15) == UNSUPPORTED

    def select(B=2, H=480, W=640, n=fake, thr=0.005, K=4096, border=4, kp=fake, sc=fake, count=fake, cand=fake, ws=fake, ws_bytes=need):
        return lib.splatraster_sp_select(B, H, W, n, thr, K, border, kp, sc, count, cand, ws, ws_bytes, None)

    assert select(B=0) == BAD and select(H=0) == BAD and select(W=0) == BAD
    assert all(select(**{k: None}) == BAD for k in ("n", "kp", "sc", "count", "cand", "ws"))
    assert select(thr=-0.001) == BAD and select(thr=float("nan")) == BAD and select(border=-1) == BAD
    assert select(K=0) == BAD and select(K=65536) == BAD and select(ws_bytes=need - 1) == BAD and select(ws=odd) == BAD
    assert select(B=1, H=1 << 16, W=1 << 15, ws_bytes=1 << 60) == UNSUPPORTED

    def sample(B=2, Hc=60, Wc=80, coarse=fake, K=4096, kp=fake, count=fake, desc=fake, ws=fake, ws_bytes=need):
        return lib.splatraster_sp_sample(B, Hc, Wc, coarse, K, kp, count, desc, ws, ws_bytes, None)

    assert sample(B=0) == BAD and sample(Hc=0) == BAD and sample(Wc=0) == BAD and sample(K=0) == BAD and sample(K=65536) == BAD
    assert all(sample(**{k: None}) == BAD for k in ("coarse", "kp", "count", "desc", "ws"))
    assert sample(ws_bytes=2 * 60 * 80 * 256 * 4 - 1) == BAD and sample(ws=odd) == BAD
    assert sample(Hc=1 << 13, Wc=1 << 12, ws_bytes=1 << 60) == UNSUPPORTED

    def dense(B=2, Hc=60, Wc=80, coarse=fake, row0=0, rows=480, out=fake, ws=fake, ws_bytes=need):
        return lib.splatraster_sp_dense_descriptors(B, Hc, Wc, coarse, row0, rows, out, ws, ws_bytes, None)

    assert dense(B=0) == BAD and dense(Hc=0) == BAD and dense(Wc=0) == BAD
    assert all(dense(**{k: None}) == BAD for k in ("coarse", "out", "ws"))
    assert dense(row0=-1) == BAD and dense(rows=0) == BAD and dense(row0=1) == BAD and dense(row0=479, rows=2) == BAD
    assert dense(out=odd) == BAD and dense(ws=odd) == BAD and dense(ws_bytes=2 * 60 * 80 * 256 * 4 - 1) == BAD


def test_host_queries_never_initialise_the_device():
    """the tile and workspace queries answer in a process that can see no device at all"""
    from splatloc_amd import _native
    _native.load()
    code = ("import ctypes as C, sys\n"
            "lib = C.CDLL(sys.argv[1])\n"
            "a, b, n = C.c_int32(0), C.c_int32(0), C.c_size_t(0)\n"
            "assert lib.splatraster_sp_nms_tile(C.byref(a), C.byref(b)) == 0\n"
            "assert lib.splatraster_sp_workspace_bytes(1, 480, 640, 4096, C.byref(n)) == 0 and n.value > 0\n"
            "print(a.value, b.value)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, _native.lib_path()], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    from splatloc_amd import superpoint
    assert tuple(int(v) for v in r.stdout.split()) == superpoint.nms_tile()


def test_python_layer_refuses_before_device_work():
    from splatloc_amd import superpoint as SP
    semi, coarse = torch.zeros(1, 65, 3, 4), torch.zeros(1, 256, 3, 4)
    for call in (lambda: SP.score_map(semi), lambda: SP.nms(torch.zeros(1, 24, 32), 4), lambda: SP.select(torch.zeros(1, 24, 32)),
                 lambda: SP.sample(coarse, torch.zeros(1, 4, 2), torch.zeros(1, dtype=torch.int32)), lambda: SP.detect(semi, coarse),
                 lambda: SP.postprocess(semi, coarse), lambda: SP.dense_descriptors(coarse), lambda: SP.sp_kp_mask(torch.zeros(24, 32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        SP.score_map(np.zeros((1, 65, 3, 4), np.float32))
    assert SP.nms_tile() == (64, 64)
