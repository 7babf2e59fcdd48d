"""Landmark selection on the MI355X (csrc/selection.hip through splatloc_amd.selection) against the reference's own numbers
(tests/golden/selection.npz) and the f64 restatement of tests/test_host_selection.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from splatloc_amd import build as B
from splatloc_amd import selection as S
from tests.test_host_selection import check_scores, golden, greedy_pick, priority_order, scores_f64

pytestmark = pytest.mark.gpu


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_device_scores_match_fixture_a():
    g = golden()
    got = _np(S.landmark_scores(g["a_points"], g["a_w2cs"], g["K"], g["a_depths"]))
    check_scores(got, g)


@pytest.mark.parametrize("num", [1, 40, 400])
def test_device_pick_from_golden_scores(num):
    g = golden()
    idx = S.select_landmarks(torch.from_numpy(g["a_points"]).cuda(), torch.from_numpy(g["a_score"]).cuda(), num)
    assert np.array_equal(g["a_points"][idx.cpu().numpy()].astype(np.float64), g[f"a_pick_{num}"])


def test_drop_in_reproduces_fixture_b():
    g = golden()
    out = S.gaussian_selectition(g["b_points"], g["b_w2cs"], g["K"], g["b_depths"], num_gs=64)
    assert out.dtype == np.float64 and out.shape == (64, 3)
    assert np.array_equal(out, g["b_pick_64"])
    # torch inputs on the device give the same answer
    dev = {k: torch.from_numpy(g[k]).cuda() for k in ("b_points", "b_w2cs", "b_depths")}
    out2 = S.gaussian_selection(dev["b_points"], dev["b_w2cs"], torch.from_numpy(g["K"]), dev["b_depths"], num_gs=64)
    assert np.array_equal(out2, g["b_pick_64"])


def test_tied_scores_follow_the_documented_order():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-50, 50, size=(3000, 3)).astype(np.float32)
    scores = rng.integers(0, 4, size=3000).astype(np.float64)        # four tied groups
    for num in (1, 7, 300):
        idx = S.select_landmarks(torch.from_numpy(pts).cuda(), torch.from_numpy(scores).cuda(), num).cpu().numpy()
        assert np.array_equal(idx, greedy_pick(pts, scores, num))
    idx = S.select_landmarks(torch.from_numpy(pts).cuda(), torch.from_numpy(scores).cuda(), 1).cpu().numpy()
    assert idx[0] == priority_order(scores)[0] == np.flatnonzero(scores == 3).max()


def _random_scene(rng, N, M):
    from tests.golden.make_golden_selection import expand_depths, look_w2c, render_mm
    w2cs, mms = [], []
    for _ in range(M):
        c = np.array([rng.uniform(1.5, 6.5), rng.uniform(1.5, 4.5), rng.uniform(1.0, 2.0)])
        w2c = look_w2c(c, rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.2))
        w2cs.append(w2c)
        mms.append(render_mm(w2c, rng, 0.05))
    pts = rng.uniform([-0.5, -0.5, -0.5], [8.5, 6.5, 3.5], size=(N, 3)).astype(np.float32)
    return pts, np.stack(w2cs), expand_depths(np.stack(mms))


def test_device_scores_match_restatement_at_scale():
    from tests.golden.make_golden_selection import K
    rng = np.random.default_rng(11)
    pts, w2cs, depths = _random_scene(rng, 200_000, 64)
    got = _np(S.landmark_scores(pts, w2cs, K, depths))
    ref = scores_f64(pts, w2cs, K, depths)
    assert np.array_equal(got["n_visible"], ref["n_visible"])
    assert np.array_equal(got["n_depth"], ref["n_depth"])
    assert (ref["n_visible"] == 0).any() and (ref["n_visible"] >= 2).mean() > 0.5
    # n_visible == 1: lmin is 0 in exact arithmetic and ~1e-16 after rounding, so the span is ~1e-8 either way
    one = ref["n_visible"] == 1
    assert np.abs(got["span"][one] - ref["span"][one]).max() <= 1e-7
    rest = ~one
    assert np.all(np.abs(got["score"][rest] - ref["score"][rest]) <= 1e-9 * np.abs(ref["score"][rest]))
    assert np.all(np.abs(got["score"][one] - ref["score"][one]) <= 1e-7)
    has = ref["n_depth"] > 0
    for k in ("depth_mean", "depth_std"):
        assert np.all(np.isnan(got[k][~has]))
        assert np.allclose(got[k][has], ref[k][has], rtol=1e-9, atol=1e-12), k


def test_device_pick_matches_cpu_greedy_at_scale():
    rng = np.random.default_rng(5)
    pts = rng.uniform([0, 0, 0], [8, 6, 3], size=(30_000, 3)).astype(np.float32)
    scores = torch.from_numpy(rng.random(30_000) * 5.0).cuda()
    idx, passes = S.select_landmarks(torch.from_numpy(pts).cuda(), scores, 1000, return_passes=True)
    assert passes >= 4
    assert np.array_equal(idx.cpu().numpy(), greedy_pick(pts, scores.cpu().numpy(), 1000))


def test_edge_cases():
    g = golden()
    pts, w2cs, K, depths = g["a_points"], g["a_w2cs"], g["K"], g["a_depths"]
    # num_gs = 1 and num_gs = N
    sc = S.landmark_scores(pts[:50], w2cs, K, depths)["score"].cpu().numpy()
    out = S.gaussian_selectition(pts[:50], w2cs, K, depths, num_gs=1)
    assert np.array_equal(out, pts[[priority_order(sc)[0]]].astype(np.float64))
    full = S.select_landmarks(pts[:50], sc, 50).cpu().numpy()
    assert sorted(full) == list(range(50)) and np.array_equal(full, greedy_pick(pts[:50], sc, 50))
    # N = 1
    one = S.gaussian_selectition(pts[:1], w2cs, K, depths, num_gs=1)
    assert np.array_equal(one, pts[:1].astype(np.float64))
    # a NaN pose is never visible; an all-hole depth map keeps no diff
    w_nan = w2cs.copy()
    w_nan[3] = np.nan
    d_hole = depths.copy()
    d_hole[5] = 0.0
    a = _np(S.landmark_scores(pts, w2cs, K, depths))
    b = _np(S.landmark_scores(pts, w_nan, K, d_hole))
    ref = scores_f64(pts, w_nan, K, d_hole)
    assert np.array_equal(b["n_visible"], ref["n_visible"]) and np.array_equal(b["n_depth"], ref["n_depth"])
    vis3 = scores_f64(pts, w2cs[3:4], K, depths[3:4])["n_visible"]
    assert np.array_equal(a["n_visible"] - b["n_visible"], vis3)
    assert np.all(np.isfinite(b["score"]))
    # too few distinct positions
    dup = np.repeat(pts[:3], 4, axis=0)
    with pytest.raises(ValueError, match="distinct"):
        S.select_landmarks(dup, np.arange(12.0), 4)
    assert S.select_landmarks(dup, np.arange(12.0), 3).shape == (3,)


def test_non_default_stream():
    g = golden()
    s = torch.cuda.Stream()
    pts = torch.from_numpy(g["a_points"]).cuda()
    w = torch.from_numpy(g["a_w2cs"]).cuda()
    d = torch.from_numpy(g["a_depths"]).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sc = S.landmark_scores(pts, w, g["K"], d)
        idx = S.select_landmarks(pts, sc["score"], 400)
    s.synchronize()
    check_scores(_np(sc), g)
    base = S.select_landmarks(pts, torch.from_numpy(g["a_score"]).cuda(), 400)
    ref = greedy_pick(g["a_points"], sc["score"].cpu().numpy(), 400)
    assert np.array_equal(idx.cpu().numpy(), ref)
    assert base.shape == idx.shape


def _usage(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in B._flags(src) if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def test_selection_kernels_use_no_scratch():
    u = _usage("selection.hip")
    assert len(u) == 7, sorted(u)
    for k, v in u.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
