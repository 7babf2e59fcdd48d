"""Landmark selection (utils/selection.py:91-157, gaussian_selectition) on the host: a vectorised numpy f64 restatement of the
score and the greedy pick, written from the semantics in INTEGRATION.md §16, against the reference's own numbers
(tests/golden/selection.npz, make_golden_selection.py); and the argument errors of splatloc_amd.selection, raised before any
device work.  The restatement is also the CPU side of tests/test_gpu_selection.py."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selection.npz")
W, H = 640, 480


def expand_depths(mm):
    """[M, 60, 80] uint16 millimetres -> [M, 480, 640] float32 metres (exact)"""
    d = np.repeat(np.repeat(mm, 8, axis=1), 8, axis=2)
    return d.astype(np.float32) / np.float32(1000.0)


def scores_f64(points, w2cs, K, depths, width=W, height=H, chunk=4096):
    """per point: n_visible, n_depth, depth_mean, depth_std, span, score (f64 from the f32 inputs, same operation order as
    the kernel: sums left to right, no contraction in numpy)"""
    out = {k: [] for k in ("n_visible", "n_depth", "depth_mean", "depth_std", "span", "score")}
    R = w2cs[:, :3, :3].astype(np.float64)
    t = w2cs[:, :3, 3].astype(np.float64)
    K = np.asarray(K, np.float64)
    M = len(w2cs)
    for c0 in range(0, len(points), chunk):
        p = points[c0:c0 + chunk].astype(np.float64)[:, None, :]          # [n, 1, 3]
        pc = [R[None, :, r, 0] * p[..., 0] + R[None, :, r, 1] * p[..., 1] + R[None, :, r, 2] * p[..., 2] + t[None, :, r]
              for r in range(3)]
        q = [K[r, 0] * pc[0] + K[r, 1] * pc[1] + K[r, 2] * pc[2] for r in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = q[0] / q[2], q[1] / q[2]
            vis = ~(pc[2] < 0.01) & (u < width) & (u > 0) & (v < height) & (v > 0)
            ui = np.where(vis, u, 0).astype(np.int64)
            vi = np.where(vis, v, 0).astype(np.int64)
        d = depths[np.arange(M)[None, :], vi, ui].astype(np.float64)
        diff = np.abs(pc[2] - d)
        kept = vis & (diff < 0.3) & (d > 0.02)
        nd = kept.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(kept, diff, 0.0).sum(1) / nd
            std = np.sqrt(np.where(kept, (diff - mean[:, None]) ** 2, 0.0).sum(1) / nd)
            e = p - t[None]
            b = [R[None, :, 0, j] * e[..., 0] + R[None, :, 1, j] * e[..., 1] + R[None, :, 2, j] * e[..., 2] for j in range(3)]
            nb = np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
            b = [x / nb for x in b]
        nv = vis.sum(1)
        Hm = np.zeros((len(p), 3, 3))
        for i in range(3):
            for j in range(3):
                Hm[:, i, j] = np.where(vis, (1.0 if i == j else 0.0) - b[i] * b[j], 0.0).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            Hm /= np.maximum(nv, 1)[:, None, None]
            ev = np.linalg.eigvalsh(Hm)
            span = np.arccos(np.clip(1.0 - 2.0 * ev[:, 0] / ev[:, 2], 0.0, 1.0))
            span = np.where(nv > 0, span, 0.0)
            a, s = 0.05 / mean, 0.05 / std
        ds = np.where(a < 2, a, 2.0) + np.where(s < 2, s, 2.0)                   # python's min(2, x): NaN -> 2
        for k, val in (("n_visible", nv), ("n_depth", nd), ("depth_mean", mean), ("depth_std", std), ("span", span),
                       ("score", ds + span)):
            out[k].append(val)
    return {k: np.concatenate(v) for k, v in out.items()}


def priority_order(scores):
    """score descending, ties the larger index first (a stable ascending sort, reversed)"""
    return np.argsort(scores, kind="stable")[::-1]


def greedy_pick(points, scores, num, radius=18.0):
    """the reference's greedy loop, vectorised per candidate; indices in pick order"""
    order = priority_order(scores)
    P = points.astype(np.float64)
    sel = [order[0]]
    L = np.zeros((num, 3))
    L[0] = P[order[0]]
    while len(sel) < num:
        assert radius > 0
        for i in order:
            d = P[i][:, None] - L[:len(sel)].T
            if np.any(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < radius):
                continue
            L[len(sel)] = P[i]
            sel.append(i)
            if len(sel) == num:
                break
        radius *= 0.5
    return np.array(sel)


def golden():
    g = dict(np.load(GOLDEN))
    g["a_depths"] = expand_depths(g["a_depth_mm"])
    g["b_depths"] = expand_depths(g["b_depth_mm"])
    return g


def check_scores(got, g, prefix="a_"):
    """the bars of fixture A: counts exact, span 1e-6 (n_visible >= 2) / 2e-3 (== 1), mean / std 1e-5 relative"""
    nv = g[prefix + "n_visible"]
    assert np.array_equal(np.asarray(got["n_visible"]), nv)
    assert np.array_equal(np.asarray(got["n_depth"]), g[prefix + "n_depth"])
    span = np.asarray(got["span"])
    m2, m1 = nv >= 2, nv == 1
    assert np.abs(span[m2] - g[prefix + "span"][m2]).max() <= 1e-6
    assert np.abs(span[m1] - g[prefix + "span"][m1]).max() <= 2e-3
    assert np.all(span[nv == 0] == 0.0)
    has = g[prefix + "n_depth"] > 0
    for k in ("depth_mean", "depth_std"):
        a, b = np.asarray(got[k]), g[prefix + k]
        assert np.all(np.isnan(a[~has])), k
        assert np.all(np.abs(a[has] - b[has]) <= 1e-5 * np.abs(b[has])), k
    # the score follows: each depth half moves by <= 2 * 1e-5, the span by its bar
    bar = np.where(m1, 2e-3, 1e-6) + 4e-5
    assert np.all(np.abs(np.asarray(got["score"]) - g[prefix + "score"]) <= bar)


def test_fixture_a_covers_the_cases():
    g = golden()
    nv, nd = g["a_n_visible"], g["a_n_depth"]
    assert (nv == 0).sum() == 1 and (nv == 1).sum() > 20 and (nv >= 2).sum() > 500
    assert (nd < nv).sum() > 100 and (nd == 0).sum() > 10
    assert g["a_depths"].shape[1:] == (480, 640) and (g["a_depth_mm"] == 0).any()
    assert len(np.unique(g["a_score"])) == len(g["a_score"])


def test_restatement_matches_reference_scores():
    g = golden()
    got = scores_f64(g["a_points"], g["a_w2cs"], g["K"], g["a_depths"])
    check_scores(got, g)


@pytest.mark.parametrize("num", [1, 40, 400])
def test_restatement_greedy_matches_reference(num):
    g = golden()
    idx = greedy_pick(g["a_points"], g["a_score"], num)
    assert np.array_equal(g["a_points"][idx].astype(np.float64), g[f"a_pick_{num}"])


def test_restatement_reproduces_fixture_b():
    g = golden()
    got = scores_f64(g["b_points"], g["b_w2cs"], g["K"], g["b_depths"])
    assert np.all(got["n_visible"] >= 2)
    assert np.array_equal(priority_order(got["score"]), priority_order(g["b_score"]))
    idx = greedy_pick(g["b_points"], got["score"], 64)
    assert np.array_equal(g["b_points"][idx].astype(np.float64), g["b_pick_64"])


def test_tie_rule_is_larger_index_first():
    s = np.array([1.0, 3.0, 3.0, 0.5, 3.0])
    assert list(priority_order(s)) == [4, 2, 1, 0, 3]


def test_argument_errors_before_device_work():
    from splatloc_amd import selection as S
    pts = np.zeros((10, 3), np.float32)
    pts[:, 0] = np.arange(10)
    w2cs = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    K = np.eye(3)
    with pytest.raises(ValueError, match="depth maps for"):
        S.landmark_scores(pts, w2cs, K, np.zeros((2, 480, 640), np.float32))
    with pytest.raises(ValueError, match="smaller than"):
        S.landmark_scores(pts, w2cs, K, np.zeros((3, 240, 320), np.float32))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        S.landmark_scores(pts[:, :2], w2cs, K, np.zeros((3, 480, 640), np.float32))
    with pytest.raises(ValueError, match=r"\[M, 4, 4\]"):
        S.landmark_scores(pts, w2cs[:, :3], K, np.zeros((3, 480, 640), np.float32))
    with pytest.raises(ValueError, match=r"K must be"):
        S.landmark_scores(pts, w2cs, np.eye(4), np.zeros((3, 480, 640), np.float32))
    for bad in (0, 11, -3):
        with pytest.raises(ValueError, match="num_gs must be"):
            S.gaussian_selectition(pts, w2cs, K, np.zeros((3, 480, 640), np.float32), num_gs=bad)
        with pytest.raises(ValueError, match="num must be"):
            S.select_landmarks(pts, np.zeros(10), bad)
    with pytest.raises(ValueError, match="scores must be"):
        S.select_landmarks(pts, np.zeros(9), 3)
    with pytest.raises(ValueError, match="radius"):
        S.select_landmarks(pts, np.zeros(10), 3, radius=0.0)
    assert S.gaussian_selection is S.gaussian_selectition
