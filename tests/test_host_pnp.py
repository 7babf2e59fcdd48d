"""Absolute pose (test.py:64-84, solve_pose) on the host: an f64 restatement of csrc/pnp.hip's sampler, P3P, scoring, trial
rule and local optimisation (include/splatraster.h), checked on planted poses; the argument errors of
splatloc_amd.pnp, raised before any device work; solve_pose's conversion against the reference's on tests/golden/pnp.npz
(make_golden_pnp.py); and the compiler's resource report of csrc/pnp.hip.  The restatement is also the CPU side of
tests/test_gpu_pnp.py and tests/test_gpu_pnp_edges.py; its premises on the cases of tests/pnp_cases.py (decisions independent
of the summation order, no residual on the threshold) are checked here."""
import math
import os

import numpy as np
import pytest

from tests.test_host_matching import _usage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp.npz")
BATCH = 1024
M64 = (1 << 64) - 1
REPLICA = {"model": "OPENCV", "width": 640, "height": 480,
           "params": [640.0 / 2.0 / 0.9999999999999999, 640.0 / 2.0 / 0.9999999999999999, (640 - 1.0) / 2.0,
                      (480 - 1.0) / 2.0, 0., 0., 0., 0.]}
SCENE12 = {"model": "OPENCV", "width": 640, "height": 480, "params": [572, 572, 320, 240, 0., 0., 0., 0.]}


# ------------------------------------------------------------------------------------------------------------- sampler
def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample(seed, trial, n):
    s = mix(seed & M64)
    t3 = (trial * 3) & M64
    i0 = mix(s ^ t3) % n
    i1 = mix(s ^ (t3 + 1)) % (n - 1)
    i1 += i1 >= i0
    i2 = mix(s ^ (t3 + 2)) % (n - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return i0, i1, i2


# ------------------------------------------------------------------------------------------------------ minimal solver
def cubic_max_root(a, b, c):
    Q = (a * a - 3.0 * b) / 9.0
    R = ((2.0 * a * a * a - 9.0 * a * b) + 27.0 * c) / 54.0
    Q3 = Q * Q * Q
    if R * R < Q3:
        th = math.acos(R / math.sqrt(Q3))
        x = -2.0 * math.sqrt(Q) * math.cos((th + 2.0 * math.pi) / 3.0) - a / 3.0
    else:
        A = -math.copysign(1.0, R) * float(np.cbrt(abs(R) + math.sqrt(R * R - Q3)))
        Bv = Q / A if A != 0.0 else 0.0
        x = (A + Bv) - a / 3.0
    for _ in range(2):
        f = ((x + a) * x + b) * x + c
        d = (3.0 * x + 2.0 * a) * x + b
        if d != 0.0:
            x = x - f / d
    return x


def quartic_roots(A4, A3, A2, A1, A0):
    big = max(abs(A3), abs(A2), abs(A1), abs(A0))
    if not (math.isfinite(A4) and math.isfinite(big) and abs(A4) > 1e-14 * big):
        return []
    b, c, d, e = A3 / A4, A2 / A4, A1 / A4, A0 / A4
    bb = b * b
    p = c - 0.375 * bb
    q = (d - 0.5 * b * c) + 0.125 * bb * b
    r = ((e - 0.25 * b * d) + 0.0625 * bb * c) - 0.01171875 * bb * bb
    m = cubic_max_root(p, 0.25 * p * p - r, -0.125 * q * q)
    ys = []
    if m > 1e-14 * (1.0 + abs(p)):
        s = math.sqrt(2.0 * m)
        h = 0.5 * p + m
        g = q / (2.0 * s)
        for sg in (-1.0, 1.0):
            bq, cq = sg * s, h - sg * g
            disc = bq * bq - 4.0 * cq
            if disc >= 0.0:
                sd = math.sqrt(disc)
                ys += [0.5 * (-bq - sd), 0.5 * (-bq + sd)]
    else:
        disc = p * p - 4.0 * r
        if disc >= 0.0:
            sd = math.sqrt(disc)
            for z in (0.5 * (-p - sd), 0.5 * (-p + sd)):
                if z >= 0.0:
                    rz = math.sqrt(z)
                    ys += [-rz, rz]
    out = []
    for y in ys:
        x = y - 0.25 * b
        for _ in range(2):
            f = (((x + b) * x + c) * x + d) * x + e
            df = ((4.0 * x + 3.0 * b) * x + 2.0 * c) * x + d
            if df != 0.0:
                x = x - f / df
        out.append(x)
    return out


def _frame(p1, p2, p3):
    d1 = [p2[k] - p1[k] for k in range(3)]
    d2 = [p3[k] - p1[k] for k in range(3)]
    n = [d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]]
    l1 = math.sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2])
    l2 = math.sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2])
    ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if not (ln > 1e-10 * l1 * l2):
        return None
    e1 = [x / l1 for x in d1]
    e3 = [x / ln for x in n]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return [[e1[k], e2[k], e3[k]] for k in range(3)]   # columns e1, e2, e3


def bearing(u, v, fx, fy, cx, cy):
    x, y = (u - cx) / fx, (v - cy) / fy
    ln = math.sqrt((x * x + y * y) + 1.0)
    return [x / ln, y / ln, 1.0 / ln]


def p3p(j, P):
    """Grunert's P3P as csrc/pnp.hip runs it: j, P 3 x 3 lists (bearings, world points); a list of 12-vectors (R row-major, t)"""
    def sq(a, b):
        d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (d0 * d0 + d1 * d1) + d2 * d2

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    a2, b2, c2 = sq(P[1], P[2]), sq(P[0], P[2]), sq(P[0], P[1])
    if not (a2 > 0.0 and b2 > 0.0 and c2 > 0.0):
        return []
    ca, cb, cg = dot(j[1], j[2]), dot(j[0], j[2]), dot(j[0], j[1])
    amc, apc, bmc, bma = (a2 - c2) / b2, (a2 + c2) / b2, (b2 - c2) / b2, (b2 - a2) / b2
    A4 = (amc - 1.0) * (amc - 1.0) - 4.0 * c2 / b2 * ca * ca
    A3 = 4.0 * ((amc * (1.0 - amc) * cb - (1.0 - apc) * ca * cg) + 2.0 * c2 / b2 * ca * ca * cb)
    A2 = 2.0 * (((((amc * amc - 1.0) + 2.0 * amc * amc * cb * cb) + 2.0 * bmc * ca * ca) - 4.0 * apc * ca * cb * cg) +
                2.0 * bma * cg * cg)
    A1 = 4.0 * ((-amc * (1.0 + amc) * cb + 2.0 * a2 / b2 * cg * cg * cb) - (1.0 - apc) * ca * cg)
    A0 = (1.0 + amc) * (1.0 + amc) - 4.0 * a2 / b2 * cg * cg
    vs = quartic_roots(A4, A3, A2, A1, A0)
    Fw = _frame(P[0], P[1], P[2])
    if Fw is None:
        return []
    out = []
    for v in vs:
        den = 2.0 * (cg - v * ca)
        if not (v > 0.0) or den == 0.0:
            continue
        u = (((amc - 1.0) * v * v - 2.0 * amc * cb * v) + 1.0 + amc) / den
        if not (u > 0.0):
            continue
        s1 = math.sqrt(b2 / ((1.0 + v * v) - 2.0 * v * cb))
        s2, s3 = u * s1, v * s1
        for _ in range(3):
            f0 = ((s1 * s1 + s2 * s2) - 2.0 * s1 * s2 * cg) - c2
            f1 = ((s1 * s1 + s3 * s3) - 2.0 * s1 * s3 * cb) - b2
            f2 = ((s2 * s2 + s3 * s3) - 2.0 * s2 * s3 * ca) - a2
            j00, j01, j02 = 2.0 * (s1 - s2 * cg), 2.0 * (s2 - s1 * cg), 0.0
            j10, j11, j12 = 2.0 * (s1 - s3 * cb), 0.0, 2.0 * (s3 - s1 * cb)
            j20, j21, j22 = 0.0, 2.0 * (s2 - s3 * ca), 2.0 * (s3 - s2 * ca)
            det = (j00 * (j11 * j22 - j12 * j21) - j01 * (j10 * j22 - j12 * j20)) + j02 * (j10 * j21 - j11 * j20)
            if not (abs(det) > 0.0):
                break
            d0 = (f0 * (j11 * j22 - j12 * j21) - j01 * (f1 * j22 - j12 * f2)) + j02 * (f1 * j21 - j11 * f2)
            d1 = (j00 * (f1 * j22 - j12 * f2) - f0 * (j10 * j22 - j12 * j20)) + j02 * (j10 * f2 - f1 * j20)
            d2 = (j00 * (j11 * f2 - f1 * j21) - j01 * (j10 * f2 - f1 * j20)) + f0 * (j10 * j21 - j11 * j20)
            s1, s2, s3 = s1 - d0 / det, s2 - d1 / det, s3 - d2 / det
        Cp = [[j[0][k] * s1 for k in range(3)], [j[1][k] * s2 for k in range(3)], [j[2][k] * s3 for k in range(3)]]
        Fc = _frame(Cp[0], Cp[1], Cp[2])
        if Fc is None:
            continue
        m = [0.0] * 12
        for r in range(3):
            for c in range(3):
                m[r * 3 + c] = (Fc[r][0] * Fw[c][0] + Fc[r][1] * Fw[c][1]) + Fc[r][2] * Fw[c][2]
        for r in range(3):
            cs = (Cp[0][r] + Cp[1][r]) + Cp[2][r]
            rp = (m[r * 3 + 0] * ((P[0][0] + P[1][0]) + P[2][0]) + m[r * 3 + 1] * ((P[0][1] + P[1][1]) + P[2][1])) + \
                m[r * 3 + 2] * ((P[0][2] + P[1][2]) + P[2][2])
            m[9 + r] = (cs - rp) / 3.0
        if all(math.isfinite(x) for x in m):
            out.append(m)
    return out


def hypotheses(p2d, p3d, intr, seed, trial):
    """(sample indices, models) of one trial"""
    fx, fy, cx, cy = intr
    idx = sample(seed, trial, len(p2d))
    j = [bearing(float(p2d[i, 0]), float(p2d[i, 1]), fx, fy, cx, cy) for i in idx]
    P = [[float(x) for x in p3d[i]] for i in idx]
    return idx, p3p(j, P)


# ------------------------------------------------------------------------------------------------------------- scoring
def residuals(m, p2d, p3d, intr):
    """(squared pixel residual, z) of every correspondence under model m, in the device's operation order"""
    fx, fy, cx, cy = intr
    X0, X1, X2 = p3d[:, 0], p3d[:, 1], p3d[:, 2]
    x = ((m[0] * X0 + m[1] * X1) + m[2] * X2) + m[9]
    y = ((m[3] * X0 + m[4] * X1) + m[5] * X2) + m[10]
    z = ((m[6] * X0 + m[7] * X1) + m[8] * X2) + m[11]
    with np.errstate(divide="ignore", invalid="ignore"):
        du = p2d[:, 0] - (fx * (x / z) + cx)
        dv = p2d[:, 1] - (fy * (y / z) + cy)
    return du * du + dv * dv, z


def inliers(m, p2d, p3d, intr, thr):
    r, z = residuals(m, p2d, p3d, intr)
    return (z > 0) & (r <= thr * thr)


def score(m, p2d, p3d, intr, thr):
    r, z = residuals(m, p2d, p3d, intr)
    ok = (z > 0) & (r <= thr * thr)
    return int(ok.sum()), float(r[ok].sum())


def better(a, b):
    """support a = (count, sum) better than b"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


# ---------------------------------------------------------------------------------------------------------- trial rule
def required_trials(k, n, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, confidence=0.9999):
    p = k / n
    if k == 0 or p < min_inlier_ratio:
        return max_num_trials
    p3 = p * p * p
    if p3 >= 1.0:
        return min_num_trials
    den = math.log(1.0 - p3)
    if not den < 0.0:
        return max_num_trials
    r = math.ceil(math.log(1.0 - confidence) / den)
    return min(max(r, min_num_trials), max_num_trials)


# ------------------------------------------------------------------------------------------------------ local refinement
def expso3(w):
    th2 = float(w @ w)
    if th2 < 1e-16:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = math.sqrt(th2)
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * K + B * (K @ K)


def normal_equations(m, mask, p2d, p3d, intr, cauchy):
    """(H [6, 6], g [6], cost) of the pixel error at m over mask (left so(3) perturbation, additive t)"""
    fx, fy, cx, cy = intr
    R, t = np.asarray(m[:9]).reshape(3, 3), np.asarray(m[9:])
    a = p3d[mask] @ R.T
    xc = a + t
    ok = xc[:, 2] > 0
    a, xc, obs = a[ok], xc[ok], p2d[mask][ok]
    iz = 1.0 / xc[:, 2]
    eu = (fx * (xc[:, 0] * iz) + cx) - obs[:, 0]
    ev = (fy * (xc[:, 1] * iz) + cy) - obs[:, 1]
    r = eu * eu + ev * ev
    au, cu = fx * iz, -fx * xc[:, 0] * iz * iz
    av, cv = fy * iz, -fy * xc[:, 1] * iz * iz
    z0 = np.zeros_like(iz)
    Ju = np.stack([cu * a[:, 1], au * a[:, 2] - cu * a[:, 0], -au * a[:, 1], au, z0, cu], 1)
    Jv = np.stack([-av * a[:, 2] + cv * a[:, 1], -cv * a[:, 0], av * a[:, 0], z0, av, cv], 1)
    w = 1.0 / (1.0 + r) if cauchy else np.ones_like(r)
    H = (Ju * w[:, None]).T @ Ju + (Jv * w[:, None]).T @ Jv
    g = (Ju * w[:, None]).T @ eu + (Jv * w[:, None]).T @ ev
    return H, g, float(np.log1p(r).sum() if cauchy else r.sum())


def apply_step(m, d):
    R = expso3(d[:3]) @ np.asarray(m[:9]).reshape(3, 3)
    return np.concatenate([R.reshape(-1), np.asarray(m[9:]) + d[3:]])


def local_optimisation(m, sup, p2d, p3d, intr, thr):
    """LO rounds as pnp_lo_kernel runs them: (model, support)"""
    m = np.asarray(m, dtype=np.float64)
    for _ in range(4):
        mask = inliers(m, p2d, p3d, intr, thr)
        cur = m.copy()
        for _ in range(10):
            H, g, _ = normal_equations(cur, mask, p2d, p3d, intr, False)
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                break
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            cur = apply_step(cur, d)
            if np.linalg.norm(d) < 1e-12:
                break
        if not np.isfinite(cur).all():
            break
        s = score(cur, p2d, p3d, intr, thr)
        if not better(s, sup):
            break
        m, sup = cur, s
    return m, sup


def refine(m, mask, p2d, p3d, intr):
    """the Cauchy-loss Levenberg-Marquardt refinement of pnp_final_kernel"""
    m = np.asarray(m, dtype=np.float64)
    H, g, cost = normal_equations(m, mask, p2d, p3d, intr, True)
    lam = 1e-4
    for _ in range(100):
        A = H + lam * np.diag(np.diag(H))
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            lam *= 10.0
            if lam > 1e16:
                break
            continue
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if np.linalg.norm(d) < 1e-10:
            break
        mn = apply_step(m, d)
        Hn, gn, cn = normal_equations(mn, mask, p2d, p3d, intr, True)
        if cn < cost:
            rel = (cost - cn) / cost
            m, H, g, cost = mn, Hn, gn, cn
            lam = max(lam * 0.1, 1e-12)
            if rel < 1e-10:
                break
        else:
            lam *= 10.0
            if lam > 1e16:
                break
    return m


def estimate_restated(p2d, p3d, intr, thr=12.0, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000,
                      confidence=0.9999, seed=0):
    """the whole estimator: dict(success, R, t, inliers, num_inliers, trials, model); model is the RANSAC model (R row-major,
    t) before the refinement, the one whose inliers are reported"""
    n = len(p2d)
    if n < 4:
        return {"success": False}
    best, sup, trials, batch = None, (-1, 0.0), 0, 0
    while True:
        bb, bs = None, None
        for k in range(BATCH):
            _, ms = hypotheses(p2d, p3d, intr, seed, batch * BATCH + k)
            for m in ms:
                s = score(m, p2d, p3d, intr, thr)
                if bb is None or better(s, bs):
                    bb, bs = m, s
        if bb is not None and better(bs, sup):
            best, sup = local_optimisation(bb, bs, p2d, p3d, intr, thr)
        trials += BATCH
        batch += 1
        req = required_trials(max(sup[0], 0), n, min_inlier_ratio, min_num_trials, max_num_trials, confidence)
        if trials >= req:
            break
    if sup[0] < 4:
        return {"success": False, "trials": trials}
    mask = inliers(best, p2d, p3d, intr, thr)
    m = refine(best, mask, p2d, p3d, intr)
    return {"success": bool(np.isfinite(m).all()), "R": m[:9].reshape(3, 3), "t": m[9:], "inliers": mask,
            "num_inliers": int(sup[0]), "trials": trials, "model": np.asarray(best, dtype=np.float64)}


# ------------------------------------------------------------------------------------------------------- planted scenes
def rotation(rng, max_deg=180.0):
    w = rng.normal(size=3)
    w *= math.radians(rng.uniform(0, max_deg)) / np.linalg.norm(w)
    return expso3(w)


def noise_for(n):
    """0.5 px keypoint noise from 500 correspondences on, none below: a few dozen points with 0.5 px noise scatter the pose by
    about 0.05 degrees at f = 320 px, so the 0.05 degree bound of the tests is only sound with the larger scenes"""
    return 0.5 if n >= 500 else 0.0


def planted_scene(seed, n, outlier_share, camera, noise=None, depth=(1.0, 6.0)):
    """n correspondences of a random pose: inliers projected with `noise` px Gaussian noise (default noise_for(n)), outliers
    moved >= 40 px in the image.  Returns (p2d, p3d, R, t, is_inlier, intrinsics, scene depth); points whose noisy residual lies within 1e-6
    relative of 11 px, 12 px or 13 px are redrawn so the threshold decisions are unambiguous.  The scene depth is the
    median camera-frame depth of the points."""
    from splatloc_amd.pnp import camera_intrinsics
    intr = camera_intrinsics(camera)
    fx, fy, cx, cy = intr
    W, H = camera["width"], camera["height"]
    noise = noise_for(n) if noise is None else noise
    rng = np.random.default_rng(seed)
    R = rotation(rng)
    t = rng.normal(size=3)
    n_out = int(round(outlier_share * n))
    p2d, p3d, inl = np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n, bool)
    k = 0
    while k < n:
        u, v = rng.uniform(0, W), rng.uniform(0, H)
        d = rng.uniform(*depth)
        xc = np.array([(u - cx) / fx * d, (v - cy) / fy * d, d])
        X = R.T @ (xc - t)
        out = k < n_out
        if out:
            while True:
                uo, vo = rng.uniform(0, W), rng.uniform(0, H)
                if (uo - u) ** 2 + (vo - v) ** 2 >= 40.0 ** 2:
                    break
            obs = np.array([uo, vo])
        else:
            obs = np.array([u, v]) + rng.normal(size=2) * noise
        r, _ = residuals(np.concatenate([R.reshape(-1), t]), obs[None], X[None], intr)
        if any(abs(r[0] - e * e) <= 1e-6 * e * e for e in (11.0, 12.0, 13.0)):
            continue
        p2d[k], p3d[k], inl[k] = obs, X, not out
        k += 1
    perm = rng.permutation(n)
    zc = (p3d @ R.T + t)[:, 2]
    return p2d[perm], p3d[perm], R, t, inl[perm], intr, float(np.median(zc))


def pose_errors(R, t, R0, t0):
    """(rotation error in degrees, translation error)"""
    c = (np.trace(np.asarray(R).T @ R0) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c)))), float(np.linalg.norm(np.asarray(t) - t0))


# --------------------------------------------------------------------------------------------------------------- tests
def test_sampler_gives_distinct_in_range_indices():
    for n in (3, 4, 5, 50, 4096, 1 << 20):
        for trial in list(range(200)) + [10 ** 9, 2 ** 40]:
            i = sample(12345, trial, n)
            assert len(set(i)) == 3 and all(0 <= x < n for x in i), (n, trial, i)
    assert mix(0) == 0xE220A8397B1DCDAF   # splitmix64's first output from state 0


def test_p3p_recovers_exact_pose():
    rng = np.random.default_rng(1)
    worst, count = 0.0, 0
    for _ in range(400):
        R0, t0 = rotation(rng), rng.normal(size=3) * 0.3
        Xc = rng.uniform(-1, 1, (3, 3)) + np.array([0.0, 0.0, 5.0])
        X = (Xc - t0) @ R0
        j = [list(x / np.linalg.norm(x)) for x in Xc]
        sols = p3p(j, [list(x) for x in X])
        assert len(sols) <= 4
        err = min(max(np.abs(np.array(m[:9]) - R0.reshape(-1)).max(), np.abs(np.array(m[9:]) - t0).max()) for m in sols)
        worst = max(worst, err)
        count += len(sols)
    assert worst <= 1e-9, worst
    assert count > 400


def test_p3p_degenerate_triplets_give_no_model():
    j = [list(np.array(v) / np.linalg.norm(v)) for v in ([0.1, 0.0, 1.0], [0.0, 0.1, 1.0], [-0.1, 0.0, 1.0])]
    assert p3p(j, [[0.0, 0.0, 5.0]] * 3) == []                                   # one repeated point
    assert p3p(j, [[0.0, 0.0, 5.0], [1.0, 1.0, 5.0], [2.0, 2.0, 5.0]]) == []     # collinear
    assert p3p(j, [[0.0, 0.0, 5.0], [0.0, 0.0, 5.0], [1.0, 0.0, 5.0]]) == []     # two equal points


def test_trial_rule_edges():
    assert required_trials(100, 100) == 1000                        # k = N: the minimum
    assert required_trials(0, 100) == 100000                        # k = 0: the maximum
    assert required_trials(0, 100, min_inlier_ratio=0.0) == 100000
    assert required_trials(9, 1000) == 100000                       # below min_inlier_ratio
    assert required_trials(10, 1000, min_inlier_ratio=0.01) == 100000   # 0.01: the formula, clipped to the maximum
    want = math.ceil(math.log(1 - 0.9999) / math.log(1 - 0.2 ** 3))
    assert required_trials(200, 1000) == want == 1147
    assert required_trials(500, 1000) == 1000
    assert required_trials(200, 1000, max_num_trials=1100) == 1100
    assert required_trials(1, 2, min_num_trials=1, confidence=0.5) == 6


@pytest.mark.parametrize("camera", [REPLICA, SCENE12], ids=["replica", "scene12"])
@pytest.mark.parametrize("n,share", [(6, 0.0), (60, 0.3), (500, 0.6)])
def test_restated_estimator_recovers_planted_pose(camera, n, share):
    p2d, p3d, R0, t0, inl, intr, depth = planted_scene(7 + n, n, share, camera)
    out = estimate_restated(p2d, p3d, intr)
    assert out["success"]
    dr, dt = pose_errors(out["R"], out["t"], R0, t0)
    assert dr < 0.05 and dt < 1e-3 * depth, (dr, dt)
    r, _ = residuals(np.concatenate([R0.reshape(-1), t0]), p2d, p3d, intr)
    assert out["inliers"][inl & (r < 121.0)].all()
    assert not out["inliers"][~inl & (r > 169.0)].any()
    assert out["num_inliers"] == int(out["inliers"].sum())


def test_argument_errors_before_device_work():
    from splatloc_amd import pnp as P
    p2, p3 = np.zeros((5, 2)), np.zeros((5, 3))
    with pytest.raises(ValueError, match="differ in length"):
        P.absolute_pose_estimation(p2, np.zeros((6, 3)), SCENE12)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        P.absolute_pose_estimation(np.zeros((5, 3)), p3, SCENE12)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        P.estimate_absolute_pose(p2, np.zeros(5), np.eye(3))
    with pytest.raises(ValueError, match="finite"):
        P.absolute_pose_estimation(np.full((5, 2), np.nan), p3, SCENE12)
    with pytest.raises(ValueError, match="finite"):
        P.estimate_absolute_pose_batch([(p2, np.full((5, 3), np.inf), np.eye(3))])
    with pytest.raises(ValueError, match="unsupported camera model"):
        P.absolute_pose_estimation(p2, p3, {"model": "RADIAL", "width": 1, "height": 1, "params": [1, 0, 0, 0, 0]})
    with pytest.raises(ValueError, match="distortion"):
        P.absolute_pose_estimation(p2, p3, dict(SCENE12, params=[572, 572, 320, 240, 0.1, 0., 0., 0.]))
    with pytest.raises(ValueError, match="params"):
        P.absolute_pose_estimation(p2, p3, {"model": "PINHOLE", "width": 1, "height": 1, "params": [1, 2, 3]})
    with pytest.raises(ValueError, match="max_error_px"):
        P.absolute_pose_estimation(p2, p3, SCENE12, max_error_px=0)
    with pytest.raises(ValueError, match="confidence"):
        P.absolute_pose_estimation(p2, p3, SCENE12, confidence=1.0)
    with pytest.raises(ValueError, match="confidence"):
        P.estimate_absolute_pose(p2, p3, np.eye(3), confidence=0.0)
    with pytest.raises(ValueError, match="min_num_trials"):
        P.absolute_pose_estimation(p2, p3, SCENE12, min_num_trials=10, max_num_trials=5)
    big = np.broadcast_to(np.zeros(2), ((1 << 20) + 1, 2))
    with pytest.raises(ValueError, match="2\\^20"):
        P.absolute_pose_estimation(big, np.broadcast_to(np.zeros(3), ((1 << 20) + 1, 3)), SCENE12)
    with pytest.raises(ValueError, match="float32 or float64"):
        P.absolute_pose_estimation(np.zeros((5, 2), np.int64), p3, SCENE12)
    with pytest.raises(ValueError, match="K must be"):
        P.estimate_absolute_pose(p2, p3, np.eye(4))


def test_hypotheses_trial_range_errors_before_any_launch():
    """ntrials above the batch and a negative trial0 are SPLATRASTER_ERR_BAD_ARG; every pointer is valid (host memory), so the
    trial range alone decides, and the call returns before it touches a device"""
    import ctypes as C
    from splatloc_amd import _native
    from splatloc_amd import pnp as P
    lib = _native.load()
    tab = (P.PnpProblem * 1)(P.PnpProblem(0, 5, 0, 572.0, 572.0, 320.0, 240.0))
    opt = P.options()
    buf = np.zeros(64)
    ptr = C.c_void_p(buf.ctypes.data)

    def call(trial0, ntrials):
        return lib.splatraster_pnp_hypotheses(1, tab, C.byref(opt), trial0, ntrials, ptr, ptr, ptr, ptr, ptr, ptr, None)
    assert call(0, BATCH + 1) == 1
    assert call(-1, 1) == 1
    assert call(0, 0) == 1
    assert call(-(2 ** 40), BATCH) == 1
    assert not buf.any()


def pytest_generate_tests(metafunc):
    if "pnp_case" in metafunc.fixturenames:   # tests/pnp_cases.py imports this module: its names are read at collection
        from tests import pnp_cases
        metafunc.parametrize("pnp_case", pnp_cases.NAMES)


def test_case_reference_preconditions(pnp_case):
    """what tests/test_gpu_pnp_edges.py relies on, for every case of tests/pnp_cases.py: the restatement runs the stated
    number of trials, its decisions do not depend on the order of its sums (reversed: inliers, count, trials and success
    identical, the pose within 1e-12), and no residual of its RANSAC model lies within 1e-6 relative of the threshold"""
    from tests import pnp_cases
    case = pnp_cases.BY_NAME[pnp_case]
    p2d, p3d, intr, K = pnp_cases.scene(pnp_case)
    assert p2d.shape == (case.n, 2) and p3d.shape == (case.n, 3)
    assert p2d.dtype == p3d.dtype == (np.float32 if case.f32 else np.float64)
    ref = pnp_cases.reference(pnp_case)
    rev = pnp_cases.reordered_case(pnp_case)
    assert ref["success"] and rev["success"]
    assert ref["trials"] == rev["trials"] == case.trials
    assert ref["num_inliers"] == rev["num_inliers"] == int(ref["inliers"].sum()) >= 4
    assert np.array_equal(ref["inliers"], rev["inliers"])
    assert np.abs(ref["R"] - rev["R"]).max() <= 1e-12
    assert np.abs(ref["t"] - rev["t"]).max() <= 1e-12
    thr2 = float(case.options.get("max_error_px", 12.0)) ** 2
    r = pnp_cases.case_residuals(pnp_case)
    assert r.shape == (case.n,) and not ref["inliers"][r > thr2].any()
    assert np.abs(r - thr2).min() > 1e-6 * thr2, np.abs(r - thr2).min() / thr2


def test_tie_scene_is_decided_by_the_residual_sum():
    """the two-pose scene of tests/pnp_cases.py: the batch's best count is shared by models of both poses, the smallest and
    the largest residual sum among them belong to different poses, and the restatement returns the pose of the smallest"""
    from tests import pnp_cases
    p2d, p3d, intr, _, first = pnp_cases.tie_scene()
    sup = pnp_cases.batch_supports(p2d, p3d, intr)
    top = max(c for c, _, _ in sup)
    tied = sorted(((s, m) for c, s, m in sup if c == top), key=lambda x: x[0])
    assert top == 20 and len(tied) >= 20
    sums = sorted({s for s, _ in tied})   # a triplet drawn twice gives the same model and sum twice
    assert len(sums) >= 20 and sums[1] - sums[0] > 1e-6 * sums[0]   # rounding cannot change which sum is the smallest
    in_lo, in_hi = (inliers(m, p2d, p3d, intr, 12.0) for m in (tied[0][1], tied[-1][1]))
    assert np.array_equal(in_lo, first) or np.array_equal(in_lo, ~first)
    assert np.array_equal(in_hi, ~in_lo)
    ref = pnp_cases.tie_reference()
    rev = pnp_cases.reordered_reference(p2d, p3d, intr, seed=pnp_cases.SEED, **pnp_cases.TIE_OPTIONS)
    assert ref["success"] and ref["trials"] == rev["trials"] == BATCH and ref["num_inliers"] == rev["num_inliers"] == 20
    assert np.array_equal(ref["inliers"], in_lo) and np.array_equal(rev["inliers"], in_lo)
    assert np.abs(ref["R"] - rev["R"]).max() <= 1e-12 and np.abs(ref["t"] - rev["t"]).max() <= 1e-12
    r = pnp_cases.ransac_residuals(ref, p2d, p3d, intr)
    assert np.abs(r - 144.0).min() > 1e-6 * 144.0


def test_fewer_than_four_points_fail_without_a_device():
    from splatloc_amd import pnp as P
    assert P.absolute_pose_estimation(np.zeros((3, 2)), np.zeros((3, 3)), SCENE12) == {"success": False}
    r, t, ret = P.solve_pose(np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), REPLICA)
    assert r is None and t is None and ret == {"success": False}


def test_quaternion_helpers_round_trip():
    from splatloc_amd import pnp as P
    rng = np.random.default_rng(3)
    for k in range(200):
        R = rotation(rng) if k else np.diag([1.0, -1.0, -1.0])
        q = P.rotmat_to_qvec(R)
        assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-15
        assert np.abs(P.qvec_to_rotmat(q) - R).max() < 1e-14
        assert np.abs(P.qvec_to_rotmat(-q) - R).max() < 1e-14


def test_solve_pose_conversion_matches_reference_fixture(monkeypatch):
    from splatloc_amd import pnp as P
    g = dict(np.load(GOLDEN))
    for k in range(int(g["count"])):
        rec = {"success": bool(g[f"c{k}_success"])}
        if rec["success"]:
            rec.update(qvec=g[f"c{k}_qvec"], tvec=g[f"c{k}_tvec"], num_inliers=int(g[f"c{k}_num_inliers"]),
                       inliers=g[f"c{k}_inliers"])
        Rw2c = P.qvec_to_rotmat(rec["qvec"]) if rec["success"] else None
        monkeypatch.setattr(P, "_absolute_pose", lambda a, b, c, _r=rec, _R=Rw2c: (_r, _R))
        r, t, ret = P.solve_pose(g[f"c{k}_kp2d"], g[f"c{k}_kp3d"], REPLICA)
        assert ret is rec
        if not rec["success"]:
            assert r is None and t is None and not bool(g[f"c{k}_ref_ok"])
            continue
        assert np.abs(r - g[f"c{k}_R"]).max() <= 1e-12, k
        assert np.abs(t - g[f"c{k}_t"]).max() <= 1e-12, k
    assert any(bool(g[f"c{k}_success"]) and g[f"c{k}_qvec"][0] < 0 for k in range(int(g["count"])))   # w < 0 is covered


def test_pnp_kernels_have_no_scratch_and_no_spills():
    usage = _usage("pnp.hip")
    assert len(usage) >= 8, sorted(usage)
    for kernel in ("pnp_hyp_kernel", "pnp_score_kernel", "pnp_best_kernel", "pnp_lo_kernel", "pnp_state_kernel",
                   "pnp_final_kernel"):
        assert any(kernel in k for k in usage), kernel
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
