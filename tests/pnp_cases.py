"""The named absolute-pose cases shared by tests/test_host_pnp.py (preconditions of the reference, on the CPU) and
tests/test_gpu_pnp_edges.py (csrc/pnp.hip against the f64 restatement): n at the 64-lane and 256-thread strides, outlier shares
that need 2, 3 and 5 batches of trials, trial limits that are no multiple of the batch, the min_inlier_ratio branch of the trial
rule, another threshold and float32 input.  No tests here."""
import collections
import functools

import numpy as np

from tests import test_host_pnp as H

SEED = 5   # the sampler seed of every case

# name, n, outlier share, keypoint noise in px, camera, options of the estimator, trials the restatement runs, float32 input
Case = collections.namedtuple("Case", "name n share noise camera options trials f32")


def _case(name, n, share, noise, camera, trials, f32=False, **options):
    return Case(name, n, share, noise, camera, options, trials, f32)


CASES = (
    _case("n4", 4, 0.0, 0.5, H.SCENE12, 1024),
    _case("n5", 5, 0.0, 0.5, H.REPLICA, 1024),
    _case("n63", 63, 0.3, 0.5, H.SCENE12, 1024),
    _case("n64", 64, 0.3, 0.5, H.REPLICA, 1024),
    _case("n65", 65, 0.3, 0.5, H.SCENE12, 1024),
    _case("n255", 255, 0.6, 0.5, H.REPLICA, 1024),
    _case("n256", 256, 0.6, 0.5, H.SCENE12, 1024),
    _case("n257", 257, 0.6, 0.5, H.REPLICA, 1024),
    _case("n1025", 1025, 0.3, 0.5, H.SCENE12, 1024),
    _case("share80", 400, 0.8, 0.5, H.SCENE12, 2048),
    _case("share85", 400, 0.85, 0.5, H.REPLICA, 3072),
    _case("share90", 300, 0.9, 0.5, H.SCENE12, 5120, max_num_trials=5000),
    _case("max1500", 200, 0.5, 0.5, H.SCENE12, 2048, min_num_trials=1500, max_num_trials=1500),   # no multiple of the batch
    _case("min1", 200, 0.5, 0.5, H.REPLICA, 1024, min_num_trials=1, max_num_trials=1),
    _case("ratio", 200, 0.7, 0.5, H.SCENE12, 3072, min_inlier_ratio=0.5, max_num_trials=3000),   # k / n < min_inlier_ratio
    _case("thr2", 200, 0.3, 1.0, H.SCENE12, 1024, max_error_px=2.0),
    _case("f32", 129, 0.3, 0.5, H.REPLICA, 1024, f32=True),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)


def intrinsics_matrix(intr):
    fx, fy, cx, cy = intr
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def scene(name):
    """(p2d, p3d, intrinsics, K) of a case: planted_scene with seed 9000 + n, built once and shared (do not modify).  The f32
    case holds float32 arrays."""
    c = BY_NAME[name]
    p2d, p3d, _, _, _, intr, _ = H.planted_scene(9000 + c.n, c.n, c.share, c.camera, noise=c.noise)
    if c.f32:
        p2d, p3d = p2d.astype(np.float32), p3d.astype(np.float32)
    return p2d, p3d, intr, intrinsics_matrix(intr)


def reference_options(options):
    """estimate_restated's names of the estimator's options"""
    return {("thr" if k == "max_error_px" else k): v for k, v in options.items()}


def _widened(name):
    p2d, p3d, intr, _ = scene(name)
    return p2d.astype(np.float64), p3d.astype(np.float64), intr


@functools.lru_cache(maxsize=None)
def reference(name):
    """estimate_restated of a case (float32 input widened to f64), computed once; do not modify"""
    p2d, p3d, intr = _widened(name)
    return H.estimate_restated(p2d, p3d, intr, seed=SEED, **reference_options(BY_NAME[name].options))


def reordered_reference(p2d, p3d, intr, **kw):
    """estimate_restated with every inlier sum (score) and every normal equation accumulated over the correspondences in
    reversed order: the two functions are wrapped, the estimator around them is the same code"""
    score, normal_equations = H.score, H.normal_equations

    def score_reversed(m, a2, a3, intr_, thr):
        return score(m, a2[::-1], a3[::-1], intr_, thr)

    def normal_equations_reversed(m, mask, a2, a3, intr_, cauchy):
        return normal_equations(m, mask[::-1], a2[::-1], a3[::-1], intr_, cauchy)
    H.score, H.normal_equations = score_reversed, normal_equations_reversed
    try:
        return H.estimate_restated(p2d, p3d, intr, **kw)
    finally:
        H.score, H.normal_equations = score, normal_equations


def reordered_case(name):
    p2d, p3d, intr = _widened(name)
    return reordered_reference(p2d, p3d, intr, seed=SEED, **reference_options(BY_NAME[name].options))


def ransac_residuals(ref, p2d, p3d, intr):
    """squared pixel residuals of the reference's RANSAC model (the model before refinement, whose inliers are reported)"""
    return H.residuals(ref["model"], np.asarray(p2d, np.float64), np.asarray(p3d, np.float64), intr)[0]


def case_residuals(name):
    return ransac_residuals(reference(name), *_widened(name))


# ---- the rule between models of equal inlier count ---------------------------------------------------------------------
# Two planted poses with 20 correspondences each in one problem, solved in a single batch (min = max = 1 trial): the models of
# either pose have 20 inliers, so the smaller residual sum decides which pose the estimator returns.  On the other cases local
# optimisation leads every model of the winning count to the same optimum and hides that rule.
TIE_SEEDS = (9040, 9041)
TIE_OPTIONS = {"min_num_trials": 1, "max_num_trials": 1}


@functools.lru_cache(maxsize=None)
def tie_scene():
    """(p2d, p3d, intrinsics, K, of_first [40] bool): the correspondences of the two poses, interleaved"""
    a, b = (H.planted_scene(s, 20, 0.0, H.SCENE12, noise=0.5) for s in TIE_SEEDS)
    perm = np.random.default_rng(TIE_SEEDS[0]).permutation(40)
    p2d, p3d = np.concatenate([a[0], b[0]])[perm], np.concatenate([a[1], b[1]])[perm]
    return p2d, p3d, a[5], intrinsics_matrix(a[5]), (np.arange(40) < 20)[perm]


def batch_supports(p2d, p3d, intr, thr=12.0, batch=0):
    """[(count, sum, model)] of every model of one batch of trials, in slot order"""
    out = []
    for k in range(batch * H.BATCH, (batch + 1) * H.BATCH):
        for m in H.hypotheses(p2d, p3d, intr, SEED, k)[1]:
            out.append(H.score(m, p2d, p3d, intr, thr) + (m,))
    return out


@functools.lru_cache(maxsize=None)
def tie_reference():
    p2d, p3d, intr, _, _ = tie_scene()
    return H.estimate_restated(p2d, p3d, intr, seed=SEED, **TIE_OPTIONS)


def pose_deviation(R, t, ref):
    """(max |R - R_ref|, max |t - t_ref| / max(1, |t_ref|)) of a device pose against the restatement's refined pose"""
    dR = float(np.abs(np.asarray(R) - ref["R"]).max())
    dt = float((np.abs(np.asarray(t) - ref["t"]) / np.maximum(1.0, np.abs(ref["t"]))).max())
    return dR, dt
