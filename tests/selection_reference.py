"""CPU side of the selection edge tests (tests/test_host_selection_edges.py, tests/test_gpu_selection_edges.py): the traced
greedy loop, a numpy emulation of the kernels' own operation sequence, exact statistics, a longdouble eigen-solver, the error
bars derived from them, and one builder per case.  Every case is made from a seed or by construction; nothing is read from
disk.  `scores_f64`, `priority_order` and `greedy_pick` stay in tests/test_host_selection.py and are imported from there.

Bars (none of them comes from the device's output; all are computed per point from the reference's values)

Counts, pick indices and n_passes are exact: the restatement performs the same correctly rounded f64 operations.

depth_mean and the variance, u = 2^-53, g(k) = k u / (1 - k u), n kept diffs d_0 .. d_{n-1}, x0 = d_0, y_k = d_k - x0,
A = mean |y_k|, Q = mean y_k^2, ybar = mean y_k.  The kernel computes
    yh_k = fl(d_k - x0) = y_k (1 + e),                                   one rounded subtraction per kept diff
    s1 = left-to-right sum of yh_k:   |s1 - sum y_k| <= g(n) sum |y_k|   (n - 1 additions and the subtraction)
    a  = fl(s1 / n):                  |a - ybar|     <= g(n + 1) A
    mean = fl(x0 + a):                |mean - m|     <= g(n + 1) A + u |x0 + a| <= g(n + 2) A + u |m|       = MEAN BAR
    s2 = left-to-right sum of fl(yh_k^2): every term carries three roundings, the sum n - 1 more:
                                      |s2 - sum y_k^2| <= g(n + 2) sum y_k^2
    q  = fl(s2 / n):                  |q - Q|        <= g(n + 3) Q
    aa = fl(a * a):                   |aa - ybar^2|  <= |a - ybar| (|a| + |ybar|) + u a^2 <= g(2 n + 4) A^2 <= g(2 n + 4) Q
    var = fl(q - aa):                 |var - V|      <= g(n + 3) Q + g(2 n + 4) Q + u |var| <= g(3 n + 9) Q
(|ybar| <= A, A^2 <= Q by Jensen, |var| <= Q (1 + ...); the clamp max(var, 0) only moves var towards V >= 0.)  The kernel
returns sqrt(var) and the tests square it again: two more roundings of a value <= Q.  VARIANCE BAR = g(3 n + 11) Q.  Where all
diffs are equal every y_k is 0, both bars' A and Q vanish and the mean bar is dropped too: x0 + 0 is exact.

Span: the clipped c = 1 - 2 lmin / lmax is compared as cos(span), against `span_reference`, within SPAN_C_BAR.
"""
from fractions import Fraction

import numpy as np

from tests.test_host_selection import greedy_pick, priority_order, scores_f64  # noqa: F401  (re-exported)

U = 2.0 ** -53
f32 = np.float32

# 4 x the largest |cos(span of scores_f64) - c(span_reference)| over jacobi_cases() and grid_case(513, 129), measured on the CPU:
#   python -c "from tests.selection_reference import measure_span_c_bar as m; print(m())"
# (the 4 x margin is the fusion suite's convention for recorded deviations: a solver as accurate that rounds differently)
SPAN_C_MEASURED = 4.440892098500626e-16
SPAN_C_BAR = 4 * SPAN_C_MEASURED


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the greedy loop, traced ---------------------------------------------------------------------------------------------------
def _near(P, L, radius):
    """[len(P), len(L)] bool: numpy's ordered norm of the f64 differences < radius"""
    d = P[:, None, :] - L[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < radius


def greedy_trace(points, scores, num, radius):
    """The reference loop (greedy_pick), also returning one record per pass: radius, start (landmarks at pass start),
    survivors (candidates not near any landmark of an earlier pass), end (landmarks at pass end), and per candidate rank
    filter_killer (index of the first earlier-pass landmark within the radius, -1 for a survivor) and pass_killer (for a
    survivor walked and rejected within the pass: the ordinal, within the pass, of the first landmark near it; -1 if taken,
    -2 if never walked because num was reached)."""
    order = priority_order(scores)
    P = points.astype(np.float64)[order]
    n = len(P)
    sel, L = [0], [P[0]]
    trace = []
    while len(sel) < num:
        assert radius > 0
        start = len(sel)
        L0 = np.array(L)
        fk = np.full(n, -1, np.int64)
        for c0 in range(0, n, 2048):
            near = _near(P[c0:c0 + 2048], L0, radius)
            fk[c0:c0 + 2048] = np.where(near.any(1), near.argmax(1), -1)
        surv = np.flatnonzero(fk < 0)
        pk = np.full(n, -2, np.int64)
        new = np.zeros((min(len(surv), num - start), 3))
        k = 0
        for j in surv:
            near = _near(P[j:j + 1], new[:k], radius)[0] if k else np.zeros(0, bool)
            if near.any():
                pk[j] = near.argmax()
                continue
            pk[j] = -1
            new[k] = P[j]
            k += 1
            sel.append(j)
            L.append(P[j])
            if len(sel) == num:
                break
        trace.append(dict(radius=radius, start=start, survivors=len(surv), end=len(sel), filter_killer=fk, pass_killer=pk,
                          surv=surv))
        radius *= 0.5
    return order[np.array(sel)], trace


# ---- numpy emulation of landmark_scores_kernel's own operation sequence ----------------------------------------------------------
class LookupStack:
    """a depth stack given by a callable (view, row, col) -> f32 (arrays in, array out); indexable like the dense one"""

    def __init__(self, lookup):
        self.lookup = lookup

    def __getitem__(self, key):
        v, r, c = np.broadcast_arrays(*key)
        return np.asarray(self.lookup(v, r, c), dtype=f32)


def scores_f64_lookup(points, w2cs, K, depth_lookup, width, height):
    """scores_f64 with the depth gather through depth_lookup(view, row, col) -> f32: the same code path, hence the same bits"""
    return scores_f64(points, w2cs, K, LookupStack(depth_lookup), width, height)


def kernel_sequence(points, w2cs, K, depths, width, height):
    """What the kernel does, in its order: views one after the other, every accumulator left to right, in f64 without
    contraction.  Returns n_visible, n_depth, the kept diffs [N, M] (NaN where not kept), the shifted one-pass mean and
    variance, and H [N, 3, 3] (already divided by n_visible)."""
    p = np.asarray(points, f32).astype(np.float64)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    K = np.asarray(K, np.float64)
    n, M = len(p), len(w2cs)
    nvis, nd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    x0, s1, s2 = np.zeros(n), np.zeros(n), np.zeros(n)
    h = {k: np.zeros(n) for k in ("00", "01", "02", "11", "12", "22")}
    diffs = np.full((n, M), np.nan)
    for v in range(M):
        m = np.asarray(w2cs[v], f32).astype(np.float64)
        R, t = m[:3, :3], m[:3, 3]
        cx, cy, cz = (R[r, 0] * px + R[r, 1] * py + R[r, 2] * pz + t[r] for r in range(3))
        q0, q1, q2 = (K[r, 0] * cx + K[r, 1] * cy + K[r, 2] * cz for r in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = q0 / q2, q1 / q2
            vis = ~(cz < 0.01) & (u < width) & (u > 0) & (w < height) & (w > 0)
            ui, wi = np.where(vis, u, 0).astype(np.int64), np.where(vis, w, 0).astype(np.int64)
            d = np.asarray(depths[np.full(n, v), wi, ui], f32).astype(np.float64)
            diff = np.abs(cz - d)
            kept = vis & (diff < 0.3) & (d > 0.02)
            x0 = np.where(kept & (nd == 0), diff, x0)
            y = diff - x0
            s1 = np.where(kept, s1 + y, s1)
            s2 = np.where(kept, s2 + y * y, s2)
            nd += kept
            diffs[kept, v] = diff[kept]
            ex, ey, ez = px - t[0], py - t[1], pz - t[2]
            bx, by, bz = (R[0, j] * ex + R[1, j] * ey + R[2, j] * ez for j in range(3))
            nb = np.sqrt(bx * bx + by * by + bz * bz)
            bx, by, bz = bx / nb, by / nb, bz / nb
            for key, val in (("00", 1.0 - bx * bx), ("01", -(bx * by)), ("02", -(bx * bz)), ("11", 1.0 - by * by),
                             ("12", -(by * bz)), ("22", 1.0 - bz * bz)):
                h[key] = np.where(vis, h[key] + val, h[key])
        nvis += vis
    with np.errstate(divide="ignore", invalid="ignore"):
        a = s1 / nd
        mean = np.where(nd > 0, x0 + a, np.nan)
        var = s2 / nd - a * a
        var = np.where(nd > 0, np.where(var > 0.0, var, 0.0), np.nan)
        H = np.zeros((n, 3, 3))
        for key, val in h.items():
            i, j = int(key[0]), int(key[1])
            H[:, i, j] = H[:, j, i] = val / nvis
    return dict(n_visible=nvis, n_depth=nd, diffs=diffs, mean=mean, var=var, H=H)


# ---- exact statistics and their bars -------------------------------------------------------------------------------------------
def _exact_sums(diffs):
    """sum and sum of squares of the f64 values as integers over the common scale 2^-1200"""
    ints = [int(Fraction(float(x)) * (1 << 1200)) for x in diffs]
    return ints, sum(ints), sum(i * i for i in ints)


def stats_exact(diffs):
    """mean and population variance of the f64 diffs as exact rationals, each rounded once to f64"""
    ints, s, ss = _exact_sums(diffs)
    n = len(ints)
    return float(Fraction(s, n << 1200)), float(Fraction(n * ss - s * s, (n * n) << 2400))


def stats_bars(diffs):
    """(mean bar, variance bar) of the module docstring for these kept diffs, in view order"""
    ints, s, _ = _exact_sums(diffs)
    n = len(ints)
    ys = [i - ints[0] for i in ints]
    A = float(Fraction(sum(abs(y) for y in ys), n << 1200))
    Q = float(Fraction(sum(y * y for y in ys), n << 2400))
    m = abs(float(Fraction(s, n << 1200)))
    return (gamma(n + 2) * A + U * m if A > 0 else 0.0), gamma(3 * n + 11) * Q


# ---- eigenvalues --------------------------------------------------------------------------------------------------------------
def jacobi_minmax(H, dtype, sweeps, converge=False):
    """cyclic Jacobi of sym3_eig_minmax, vectorised over the leading axis, in `dtype`.  converge=False is the kernel's loop
    (stop when the off-diagonal sum is exactly 0, at most `sweeps`); converge=True also stops once the off-diagonal part is
    below 1e-40 of the trace, far under the unit roundoff."""
    a = {k: np.array(H[:, int(k[0]), int(k[1])], dtype=dtype) for k in ("00", "01", "02", "11", "12", "22")}
    one = dtype(1)
    for _ in range(sweeps):
        off = np.abs(a["01"]) + np.abs(a["02"]) + np.abs(a["12"])
        todo = off != 0
        if converge:
            todo &= off > dtype(1e-40) * (np.abs(a["00"]) + np.abs(a["11"]) + np.abs(a["22"]))
        if not todo.any():
            break
        for pp, qq, pq, pk, qk in (("00", "11", "01", "02", "12"), ("00", "22", "02", "01", "12"),
                                   ("11", "22", "12", "01", "02")):
            app, aqq, apq, apk, aqk = a[pp], a[qq], a[pq], a[pk], a[qk]
            act = todo & (apq != 0)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (aqq - app) / (dtype(2) * apq)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                new = (app - t * apq, aqq + t * apq, np.zeros_like(apq), c * apk - s * aqk, s * apk + c * aqk)
            for key, val in zip((pp, qq, pq, pk, qk), new):
                a[key] = np.where(act, val, a[key])
    lmin = np.minimum(a["00"], np.minimum(a["11"], a["22"]))
    lmax = np.maximum(a["00"], np.maximum(a["11"], a["22"]))
    return lmin, lmax


def _clip_c(lmin, lmax, dtype):
    with np.errstate(divide="ignore", invalid="ignore"):
        c = dtype(1) - dtype(2) * lmin / lmax
    return np.where(c < 0, dtype(0), np.where(c > 1, dtype(1), c))


def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def span_reference(H):
    """clipped c = clip(1 - 2 lmin / lmax, 0, 1) and acos(c) of the symmetric 3x3 matrices H [n, 3, 3]: a cyclic Jacobi run to
    convergence in np.longdouble (64-bit mantissa), each result rounded once to f64"""
    assert have_longdouble()
    ld = np.longdouble
    c = _clip_c(*jacobi_minmax(np.asarray(H), ld, 64, converge=True), ld)
    return c.astype(np.float64), np.arccos(c).astype(np.float64)


def span_kernel(H):
    """the kernel's own solver sequence in f64: c and acos(c)"""
    c = _clip_c(*jacobi_minmax(np.asarray(H), np.float64, 16), np.float64)
    return c, np.arccos(c)


def span_bar_from_c(c_ref):
    """the span error implied by an error of SPAN_C_BAR in c"""
    lo, hi = np.clip(c_ref - SPAN_C_BAR, 0, 1), np.clip(c_ref + SPAN_C_BAR, 0, 1)
    return np.maximum(np.abs(np.arccos(lo) - np.arccos(c_ref)), np.abs(np.arccos(hi) - np.arccos(c_ref)))


def min2(x):
    """python's min(2, x), NaN -> 2"""
    with np.errstate(invalid="ignore"):
        return np.where(x < 2, x, 2.0)


def reference_and_bars(points, w2cs, K, depths, width, height):
    """Per point: the exact counts (restatement), mean / var from stats_exact, c / span from span_reference, the score from
    those, and every bar.  The span fields are None without a 64-bit-mantissa longdouble."""
    ks = kernel_sequence(points, w2cs, K, depths, width, height)
    n = len(points)
    mean, var, dm, dv = (np.full(n, np.nan) for _ in range(4))
    for i in range(n):
        d = ks["diffs"][i]
        d = d[~np.isnan(d)]
        if len(d):
            mean[i], var[i] = stats_exact(d)
            dm[i], dv[i] = stats_bars(d)
    out = dict(n_visible=ks["n_visible"], n_depth=ks["n_depth"], mean=mean, var=var, mean_bar=dm, var_bar=dv, ks=ks,
               c=None, span=None)
    if not have_longdouble():
        return out
    seen = ks["n_visible"] > 0
    c, span = np.ones(n), np.zeros(n)
    if seen.any():
        c[seen], span[seen] = span_reference(ks["H"][seen])
    angle = seen & (c < 1 - 1e-6)                       # where the angle itself is compared, at 1e-9 relative
    dspan = np.where(angle, 1e-9 * span, np.where(seen, span_bar_from_c(c), 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(var)
        ds = np.maximum(np.abs(np.sqrt(np.maximum(var - dv, 0)) - std), np.abs(np.sqrt(var + dv) - std))
        half = lambda m, e: np.abs(min2(0.05 / (m - e)) - min2(0.05 / (m + e)))  # noqa: E731
        score = min2(0.05 / mean) + min2(0.05 / std) + span
        # a bar wider than the value itself (m - e <= 0) bounds nothing: the half can then move by its whole range
        bar = np.where(mean - dm > 0, half(mean, dm), 2.0) + np.where((std - ds > 0) | (ds == 0), half(std, ds), 2.0) + dspan
    bar = np.where(np.isnan(mean), dspan, bar)          # no diff kept: both halves are exactly 2
    out.update(c=c, span=span, angle=angle, span_bar=dspan, std=std, std_bar=ds, score=score, score_bar=bar)
    return out


def check_device_scores(got, ref, what=""):
    """the comparisons of group A: `got` the device's dict as numpy, `ref` from reference_and_bars.  Returns the largest
    err / bar ratio per quantity (for printing)."""
    assert np.array_equal(got["n_visible"], ref["n_visible"]), what
    assert np.array_equal(got["n_depth"], ref["n_depth"]), what
    has = ref["n_depth"] > 0
    worst = {}
    assert np.all(np.isnan(got["depth_mean"][~has])) and np.all(np.isnan(got["depth_std"][~has])), what
    for name, err, bar in (("mean", np.abs(got["depth_mean"] - ref["mean"])[has], ref["mean_bar"][has]),
                           ("var", np.abs(got["depth_std"] ** 2 - ref["var"])[has], ref["var_bar"][has])):
        assert np.all(err <= bar), (what, name, err.max(), bar[err > bar])
        worst[name] = float(np.max(err[bar > 0] / bar[bar > 0])) if (bar > 0).any() else 0.0
    unseen = ref["n_visible"] == 0
    assert np.all(got["span"][unseen] == 0.0), what
    if ref["c"] is None:
        return worst
    seen = ~unseen
    err = np.abs(np.cos(got["span"]) - ref["c"])[seen]
    assert np.all(err <= SPAN_C_BAR), (what, "c", err.max())
    worst["c"] = float(err.max() / SPAN_C_BAR) if seen.any() else 0.0
    ang = ref["angle"]
    assert np.all(np.abs(got["span"] - ref["span"])[ang] <= 1e-9 * ref["span"][ang]), (what, "span")
    err = np.abs(got["score"] - ref["score"])
    assert np.all(err <= ref["score_bar"]), (what, "score", err.max())
    return worst


# ---- scenes for the score tests -------------------------------------------------------------------------------------------------
def pinhole(width, height, f=None):
    f = float(f if f is not None else max(width, height))
    return np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1]], np.float64)


def look_w2c(centre, target, roll=0.0):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0])
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    x, y = np.cos(roll) * x + np.sin(roll) * y, -np.sin(roll) * x + np.cos(roll) * y
    R = np.stack([x, y, z])
    w = np.eye(4)
    w[:3, :3], w[:3, 3] = R, -R @ centre
    return w.astype(f32)


def room_case(seed, N, M, width, height, K=None, stack_hw=None, poison=None):
    """N points in a 2 m box, M cameras about 3 m away looking roughly at it (some looking away); depth maps between 2 and 4 m
    with holes, so that visible, invisible, kept and dropped pairs all occur.  stack_hw > (height, width) embeds the maps in
    a larger stack whose outside pixels hold `poison`."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, size=(N, 3)).astype(f32)
    w2cs = np.zeros((M, 4, 4), f32)
    for v in range(M):
        d = rng.normal(size=3)
        c = 3.0 * d / np.linalg.norm(d)
        target = rng.uniform(-1.5, 1.5, size=3) if v % 5 != 4 else c * 2.0
        w2cs[v] = look_w2c(c, target, rng.uniform(0, 2 * np.pi))
    sh, sw = stack_hw or (height, width)
    depths = np.full((M, sh, sw), poison if poison is not None else 0.0, f32)
    win = rng.uniform(2.0, 4.0, size=(M, height, width)).astype(f32)
    win[rng.random(win.shape) < 0.1] = 0.0
    depths[:, :height, :width] = win
    return dict(points=pts, w2cs=w2cs, K=pinhole(width, height) if K is None else np.asarray(K, np.float64), depths=depths,
                width=width, height=height)


GRID_N = (1, 255, 256, 257, 513)
GRID_M = (0, 1, 63, 64, 65, 128, 129)


def grid_case(N, M):
    return room_case(1000 * N + M, N, M, 40, 30)


GENERAL_K = np.array([[33.0, 0.75, 19.5], [0.0, 31.0, 14.25], [1e-3, -2e-3, 1.1]])
ZERO_ROW_K = np.array([[32.0, 0.5, 20.0], [0.0, 32.0, 15.0], [0.0, -0.5, 1.0]])


def general_k_case(K=GENERAL_K):
    """skew and a third row that is not (0, 0, 1); the last points sit where q2 = K[2] . (cx, cy, cz) is <= 0 (with ZERO_ROW_K
    exactly 0 for the very last) in view 0, the identity"""
    s = room_case(77, 300, 9, 40, 30, K=K)
    s["w2cs"][0] = np.eye(4, dtype=f32)
    s["points"][-4:] = np.array([[0.0, 20.0, 0.02], [-3.0, 30.0, 0.03], [0.5, 40.0, 0.05], [1.0, 2.0, 1.0]], f32)
    return s


def q2_view0(s):
    p = s["points"].astype(np.float64)
    return s["K"][2, 0] * p[:, 0] + s["K"][2, 1] * p[:, 1] + s["K"][2, 2] * p[:, 2]


IMAGE_SHAPES = ((1, 1), (1, 37), (37, 1), (641, 479))


def image_case(width, height):
    return room_case(500 + width, 257, 5, width, height)


def crop_case():
    """a 40 x 30 window of a 53 x 47 stack; outside pixels hold 3.0, which every diff test would keep"""
    return room_case(9, 257, 5, 40, 30, stack_hw=(47, 53), poison=3.0)


# ---- threshold cases: identity pose, power-of-two intrinsics, every quantity exact in f64 ------------------------------------------
TW, TH = 8, 4
TK = np.array([[4.0, 0, 4.0], [0, 4.0, 2.0], [0, 0, 1.0]])


def _at(col, row, z):
    """the f32 point that projects to (col, row) exactly at depth z under TK and the identity"""
    z = float(z)
    p = np.array([(col - 4.0) * z / 4.0, (row - 2.0) * z / 4.0, z])
    assert np.array_equal(p.astype(f32).astype(np.float64), p), (col, row, z)
    return p.astype(f32)


def threshold_case():
    """One identity view over an 8 x 4 map whose pixel k = row * 8 + col holds the distinct depth 1 + k / 128, so the kept
    diff of a point at z = 1 names the pixel it read.  Four pixels hold the threshold depths instead.  Returns the scene and,
    per point, (name, n_visible, n_depth, depth_mean or None) worked out by hand."""
    lo, hi = f32(0.01), np.nextafter(f32(0.01), f32(1))
    d02, d02s = f32(0.02), np.nextafter(f32(0.02), f32(1))
    d07, d07s = f32(0.7), np.nextafter(f32(0.7), f32(1))
    depth = (1.0 + np.arange(TW * TH, dtype=np.float64).reshape(TH, TW) / 128.0).astype(f32)
    depth[1, 1], depth[1, 2], depth[2, 1], depth[2, 2] = d02, d02s, d07, d07s
    pix = lambda r, c: (r * TW + c) / 128.0  # noqa: E731
    rows = [
        ("cz = f32(0.01) widens below 0.01: invisible", _at(4.0, 2.0, lo), 0, 0, None),
        ("cz = succ f32(0.01): visible, pixel (2, 4) is 1.15625 m away", _at(4.0, 2.0, hi), 1, 0, None),
        ("d = f32(0.02) widens below 0.02: dropped", _at(1.5, 1.5, 0.25), 1, 0, None),
        ("d = succ f32(0.02): kept", _at(2.5, 1.5, 0.25), 1, 1, 0.25 - float(d02s)),
        ("cz = 1, d = f32(0.7): diff >= 0.3, dropped", _at(1.5, 2.5, 1.0), 1, 0, None),
        ("cz = 1, d = succ f32(0.7): diff < 0.3, kept", _at(2.5, 2.5, 1.0), 1, 1, 1.0 - float(d07s)),
        ("u == 0: excluded", _at(0.0, 0.5, 1.0), 0, 0, None),
        ("u == W: excluded", _at(8.0, 0.5, 1.0), 0, 0, None),
        ("v == 0: excluded", _at(0.5, 0.0, 1.0), 0, 0, None),
        ("v == H: excluded", _at(0.5, 4.0, 1.0), 0, 0, None),
        ("u = W - 2^-20 reads column W - 1", _at(8.0 - 2.0 ** -20, 0.5, 1.0), 1, 1, pix(0, 7)),
        ("0 < v < 1 reads row 0", _at(5.5, 2.0 ** -20, 1.0), 1, 1, pix(0, 5)),
        ("v = H - 2^-20 reads row H - 1", _at(3.5, 4.0 - 2.0 ** -20, 1.0), 1, 1, pix(3, 3)),
        ("u = 2^-20 reads column 0", _at(2.0 ** -20, 3.5, 1.0), 1, 1, pix(3, 0)),
        ("u = 6.999.. truncates to column 6", _at(7.0 - 2.0 ** -20, 0.5, 1.0), 1, 1, pix(0, 6)),
    ]
    assert float(lo) < 0.01 < float(hi) and float(d02) < 0.02 < float(d02s)
    assert abs(1.0 - float(d07)) >= 0.3 > abs(1.0 - float(d07s))
    scene = dict(points=np.stack([r[1] for r in rows]), w2cs=np.eye(4, dtype=f32)[None], K=TK, depths=depth[None], width=TW,
                 height=TH)
    return scene, [(r[0], r[2], r[3], r[4]) for r in rows]


def permuted_threshold_case():
    """the same points seen by the identity and by two axis-permuting poses (camera axes = world (y, z, x) and (z, x, y))"""
    scene, _ = threshold_case()
    perm = np.zeros((3, 4, 4), f32)
    perm[0] = np.eye(4)
    perm[1, :3, :3] = [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
    perm[2, :3, :3] = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    perm[1:, 3, 3] = 1
    perm[1, :3, 3] = [0.0, 0.0, 2.0]
    perm[2, :3, 3] = [0.0, 0.0, 1.0]
    return dict(scene, w2cs=perm, depths=np.repeat(scene["depths"], 3, axis=0))


# ---- Jacobi cases: the point at the origin, every view at t = (0, 0, 1), so b = -(third row of R) --------------------------------
def _view_along(b):
    """w2c whose third rotation row is -b / |b|: the origin is seen at the principal point, one metre away"""
    z = -np.asarray(b, np.float64)
    z = z / np.linalg.norm(z)
    k = int(np.argmin(np.abs(z)))
    x = np.cross(z, np.eye(3)[k])
    x = x / np.linalg.norm(x)
    w = np.eye(4)
    w[:3, :3] = np.stack([x, np.cross(z, x), z])
    w[2, 3] = 1.0
    w = w.astype(f32)
    w[np.abs(w) < 1e-12] = 0.0
    return w


def jacobi_cases():
    ex, ey, ez = np.eye(3)
    th = 0.7
    sets = {
        "diagonal": [ex, ey, ez, ex],
        "isotropic": [ex, -ex, ey, -ey, ez, -ez],
        "rank-1 complement": [np.array([0.3, -0.5, 0.81])] * 3,
        "single off-diagonal": [np.array([np.cos(th), np.sin(th), 0.0]), ez, ex],
        "two nearly equal": [ex, np.array([np.sin(1e-7), np.cos(1e-7), 0.0]), ez, ez, ez],
        "general": [np.array([0.2, 0.1, 1.0]), np.array([-0.4, 0.3, 0.8]), np.array([0.9, 0.1, -0.2])],
    }
    out = {}
    for name, bs in sets.items():
        w2cs = np.stack([_view_along(b) for b in bs])
        out[name] = dict(points=np.zeros((1, 3), f32), w2cs=w2cs, K=pinhole(8, 8), depths=np.ones((len(bs), 8, 8), f32), width=8,
                         height=8)
    return out


def measure_span_c_bar():
    """regenerates SPAN_C_MEASURED"""
    worst = 0.0
    for s in list(jacobi_cases().values()) + [grid_case(513, 129)]:
        a = scores_f64(s["points"], s["w2cs"], s["K"], s["depths"], s["width"], s["height"])
        ks = kernel_sequence(s["points"], s["w2cs"], s["K"], s["depths"], s["width"], s["height"])
        seen = ks["n_visible"] > 0
        c, _ = span_reference(ks["H"][seen])
        worst = max(worst, float(np.abs(np.cos(a["span"][seen]) - c).max()))
    return worst


# ---- statistics cases: identity poses over the principal pixel of a 4 x 4 image -----------------------------------------------------
def _stat_scene(tz, d, pz=1.0):
    M = len(tz)
    w2cs = np.tile(np.eye(4, dtype=f32), (M, 1, 1))
    w2cs[:, 2, 3] = np.asarray(tz, f32)
    assert np.array_equal(w2cs[:, 2, 3].astype(np.float64), np.asarray(tz, np.float64))
    depths = np.broadcast_to(np.asarray(d, f32).reshape(-1, 1, 1), (M, 4, 4)).copy()
    return dict(points=np.array([[0, 0, pz]], f32), w2cs=w2cs, K=pinhole(4, 4, 4.0), depths=depths, width=4, height=4)


def statistics_cases():
    """name -> (scene, property): 'equal' (all kept diffs bit-equal), or the expected n_depth"""
    out = {}
    for nd in (1, 2, 65):
        out[f"equal x {nd}"] = (_stat_scene(np.zeros(nd), np.full(nd, 0.875)), "equal")
    # cz alternates between 0.1875 and 0.1875 + 2^-55, d = 0.0625: diffs 0.125 and 0.125 + one ulp
    out["one ulp apart"] = (_stat_scene(np.tile([0.0, 2.0 ** -55], 8), np.full(16, 0.0625), pz=0.1875), 16)
    d = np.zeros(129)
    d[77] = 0.875
    out["1 kept of 129"] = (_stat_scene(np.zeros(129), d), 1)
    # cz = 1 + j 2^-33 (j <= 8: a spread of 9.3e-10), d = f32(0.7001): diffs about 0.2999
    j = np.random.default_rng(4).integers(0, 9, size=65)
    out["0.2999, spread 1e-9"] = (_stat_scene(j * 2.0 ** -33, np.full(65, 0.7001)), 65)
    return out


# ---- large offsets ------------------------------------------------------------------------------------------------------------
BIG = dict(M=9, H=16384, W=16384, f=8192.0, fill=0.0)


def big_case():
    """a 9 x 16384 x 16384 stack (2.4e9 elements: offsets beyond 2^31) that is `fill` (a hole) everywhere but at the marked
    pixels, which hold depths that keep the diff.  View k is shifted by 16 k pixels in x.  Returns points, w2cs, K, and the
    marks {(view, row, col): depth}: the pixels the points are predicted to read in the first and the last view."""
    W, H, M, f = BIG["W"], BIG["H"], BIG["M"], BIG["f"]
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    cols = np.array([0.5, 5.5, 8192.5, 16000.5, 16383.5 - 16 * (M - 1), 100.5, 16300.5])
    rows = np.array([0.5, 16000.5, 8191.5, 16383.5, 16383.5, 16382.5, 3.5])
    pts = np.stack([(cols - W / 2) / f, (rows - H / 2) / f, np.ones(len(cols))], 1)
    assert np.array_equal(pts.astype(f32).astype(np.float64), pts)
    w2cs = np.tile(np.eye(4, dtype=f32), (M, 1, 1))
    w2cs[:, 0, 3] = 16.0 * np.arange(M) / f
    marks = {}
    for v in (0, M - 1):
        for i, (c, r) in enumerate(zip(cols, rows)):
            col = int(c + 16 * v)
            if col < W:
                marks[(v, int(r), col)] = f32(1.0 - (i + 1) / 64.0 - v / 1024.0)
    return pts.astype(f32), w2cs, K, marks


def big_lookup(marks):
    def lookup(v, r, c):
        out = np.full(np.shape(v), BIG["fill"], f32)
        for (mv, mr, mc), d in marks.items():
            out[(v == mv) & (r == mr) & (c == mc)] = d
        return out
    return lookup


# ---- order cases --------------------------------------------------------------------------------------------------------------
def lattice_points(N):
    """distinct points of the integer lattice, exact in f32; with radius 0.25 no candidate is near another"""
    i = np.arange(N, dtype=np.int64)
    return np.stack([i % 256, (i // 256) % 256, i // 65536], 1).astype(f32)


def special_scores(N=3000, seed=8):
    bits = lambda b: np.array([b], np.uint64).view(np.float64)[0]  # noqa: E731
    one = 1.0
    pool = [np.inf, -np.inf, bits(0x7ff8000000000000), bits(0xfff8000000000000), bits(0x7ff8000000000001),
            bits(0x7ff0000000000001), bits(0xfff4000000abcdef), bits(0x7fffffffffffffff), 0.0, -0.0, 5e-324, -5e-324,
            one, -one, np.nextafter(one, 2), np.nextafter(one, 0), np.nextafter(-one, 0), np.nextafter(-one, -2),
            # equal high words, different low words; equal low words, different high words
            bits(0x4000000000000001), bits(0x4000000000000002), bits(0x40000000ffffffff), bits(0x4000000100000000),
            bits(0x4000000200000000), bits(0x4010000000000001), bits(0xc000000000000001), bits(0xc000000000000002),
            bits(0xc000000100000000), bits(0xc010000000000001), -2.5, -2.25, -1e300, 1e300, 2.2250738585072014e-308,
            -2.2250738585072014e-308]
    rng = np.random.default_rng(seed)
    s = np.array(pool, np.float64)[rng.integers(0, len(pool), size=N)]
    s[:len(pool)] = pool                                    # every value at least once
    return s[rng.permutation(N)]


SORT_SIZES = (524_288, 524_289, 1_048_576, 1_048_577, 2048 * 2048 + 1)


def tied_scores(N, seed=0):
    rng = np.random.default_rng(seed + N)
    s = rng.integers(0, 50, size=N).astype(np.float64)
    where = rng.choice(N, size=40, replace=False)
    s[where] = 49.0 + rng.random(40)                        # a few distinct doubles at the top, and some below
    s[where[:10]] -= 30.0
    return s


# ---- pick cases: dict(points, scores, num, radius, want) --------------------------------------------------------------------------
def _shuffled(points, scores, seed):
    perm = np.random.default_rng(seed).permutation(len(points))
    return np.ascontiguousarray(np.asarray(points, f32)[perm]), np.asarray(scores, np.float64)[perm]


def many_landmarks_case(num=5000):
    """18^3 sites at spacing 1, each with a twin 0.125 away; radius 0.5: pass 1 takes one of every pair, in priority order"""
    g = np.arange(18, dtype=np.float64)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([sites, sites + [0.125, 0, 0]])
    rng = np.random.default_rng(10)
    p, s = _shuffled(pts, rng.random(len(pts)), 11)
    return dict(points=p, scores=s, num=num, radius=0.5)


CHUNK_SURVIVORS = (1023, 1024, 1025, 2049)


def chunk_far_case(S, num=None):
    """pass 1 at radius 0.5 over S + 1 lattice points: S survivors, mutually far, every one taken (until num)"""
    pts = lattice_points(S + 1)
    s = np.random.default_rng(S).random(S + 1)
    p, s = _shuffled(pts, s, S + 1)
    return dict(points=p, scores=s, num=S + 1 if num is None else num, radius=0.5)


def chunk_near_case(S):
    """The first landmark far away; then S survivors in clusters of 1024 by priority, each cluster within the radius of its
    first member and the clusters 10 apart: every chunk yields one landmark in pass 1 (radius 2).  One landmark more than
    that is asked for, so the later chunks' kills are what the next passes build on."""
    rng = np.random.default_rng(S)
    nch = -(-S // 1024)
    k = np.arange(S)
    pts = np.zeros((S + 1, 3))
    pts[0] = [-100, 0, 0]
    pts[1:, 0] = 10.0 * (k // 1024) + rng.permutation(1024)[k % 1024] * 2.0 ** -10
    scores = np.concatenate([[10.0], 5.0 - (k // 1024) + rng.random(S) * 0.5])
    p, s = _shuffled(pts, scores, S + 7)
    return dict(points=p, scores=s, num=1 + nch + 1, radius=2.0)


FILTER_COUNTS = (255, 256, 257, 513)


def filter_case(L):
    """Pass 1 (radius 2) takes L anchors 4 apart, in priority order.  In pass 2 (radius 1) the 300 close satellites of the
    first anchor and of the last one are killed by the filter (by landmark 0 and by landmark L - 1: the first and the last LDS
    batch), as is every anchor by itself; far satellites (1.5 from their anchor) survive and are taken."""
    k = np.arange(L)
    anchors = np.stack([4.0 * (k % 32), 4.0 * (k // 32), np.zeros(L)], 1)
    close = np.zeros((300, 3))
    close[:, 1] = (np.arange(300) + 1) * 2.0 ** -10
    far = anchors[::17] + [1.5, 0, 0]
    pts = np.concatenate([anchors, anchors[0] + close, anchors[-1] + close, far])
    rng = np.random.default_rng(L)
    scores = np.concatenate([1000.0 - k, 8.0 + rng.random(300), 6.0 + rng.random(300), rng.random(len(far))])
    p, s = _shuffled(pts, scores, L + 3)
    return dict(points=p, scores=s, num=L + len(far) - 2, radius=2.0)


def exact_lattice_case(under):
    """3^3 points at {0, s, 2 s}^3 with radius 0.25: s = 0.25 (strict <: nobody is near, all taken in pass 1) or the f32
    just under it (axis neighbours are rejected in pass 1)"""
    s = np.nextafter(f32(0.25), f32(0)) if under else f32(0.25)
    v = np.array([0.0, s, s * f32(2)], f32)
    pts = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    p, sc = _shuffled(pts, np.random.default_rng(2).random(27), 3)
    return dict(points=p, scores=sc, num=27, radius=0.25)


def _fma(a, b, c):
    """round(a * b + c) once, exactly (rational arithmetic)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def distance_variants(a, b):
    """the distance of two f32 points: numpy's order sqrt((dx^2 + dy^2) + dz^2); the two FMA chains a contracting compiler
    may form for that expression; and the association dx^2 + (dy^2 + dz^2)"""
    dx, dy, dz = (float(x) - float(y) for x, y in zip(a, b))
    s = np.sqrt
    return dict(numpy=float(s((dx * dx + dy * dy) + dz * dz)),
                fma_xy=float(s(_fma(dz, dz, _fma(dx, dx, dy * dy)))),
                fma_yx=float(s(_fma(dz, dz, _fma(dy, dy, dx * dx)))),
                assoc=float(s(dx * dx + (dy * dy + dz * dz))))


_PAIRS = {}


def rounding_pairs(count=3, seed=21):
    """f32 pairs whose numpy-ordered distance is strictly larger than under either FMA chain and under the other association"""
    if (count, seed) not in _PAIRS:
        _PAIRS[count, seed] = _find_rounding_pairs(count, seed)
    return _PAIRS[count, seed]


def _find_rounding_pairs(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        a = (rng.uniform(-50, 50, 3) * 10.0 ** rng.uniform(-3, 0, 3)).astype(f32)
        b = (rng.uniform(-50, 50, 3) * 10.0 ** rng.uniform(-3, 0, 3)).astype(f32)
        d = distance_variants(a, b)
        if max(d["fma_xy"], d["fma_yx"], d["assoc"]) < d["numpy"]:
            out.append((a, b, d))
    return out


def rounding_case(a, b, d_np, k):
    """Two clusters: a (the top score) and b, which lies exactly d_np from it, so in the pass at radius d_np (pass k + 1 of
    a start at d_np 2^k) numpy's strict < takes b.  A third point 2^-4 d_np beyond b follows b in priority: it is taken in
    that pass only if b was not."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    c = (b64 + (b64 - a64) * 2.0 ** -4).astype(f32)
    far = (a64 + 64.0 * d_np * np.array([[1, 0, 0], [0, 1, 0]])).astype(f32)
    pts = np.stack([a, b, c, far[0], far[1]])
    return dict(points=pts, scores=np.array([9.0, 5.0, 4.0, 8.0, 7.0]), num=4, radius=d_np * 2.0 ** k)


def duplicates_case():
    """6 distinct positions; two of them twice with different scores, one as (+0, 1, 2) and (-0, 1, 2)"""
    pts = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [3, 0, 0], [0.0, 1, 2], [-0.0, 1, 2], [5, 5, 5], [0, 3, 0], [1, 1, 1]], f32)
    scores = np.array([1.0, 7.0, 2.0, 3.0, 4.0, 6.0, 5.0, 8.0, 0.5])
    return dict(points=pts, scores=scores, num=6, radius=1.0, distinct=6, losers=[3, 2, 4])


def long_pass_case():
    """5 points 1e-30 apart on a line and one a metre away: about 100 halvings of 18 before the line separates"""
    pts = np.zeros((6, 3), f32)
    pts[:5, 0] = np.arange(5, dtype=f32) * f32(1e-30)
    pts[5] = [1, 0, 0]
    return dict(points=pts, scores=np.array([3.0, 1.0, 5.0, 2.0, 4.0, 0.0]), num=6, radius=18.0)


def pick_builders():
    """name -> builder of every group C case (each is run twice on the device: the runs must be bit-identical)"""
    out = {f"many landmarks, num {n}": (lambda n=n: many_landmarks_case(n)) for n in (5000, 4096, 4097, 4098)}
    for S in CHUNK_SURVIVORS:
        out[f"chunk far {S}"] = lambda S=S: chunk_far_case(S)
        out[f"chunk near {S}"] = lambda S=S: chunk_near_case(S)
    out["num at first of chunk 2"] = lambda: chunk_far_case(2049, num=1 + 1025)
    out["num inside chunk 1"] = lambda: chunk_far_case(1023, num=1 + 500)
    for L in FILTER_COUNTS:
        out[f"filter {L}"] = lambda L=L: filter_case(L)
    out["lattice at r"] = lambda: exact_lattice_case(False)
    out["lattice under r"] = lambda: exact_lattice_case(True)
    for i in range(3):
        out[f"rounding pair {i}"] = lambda i=i: rounding_case(*rounding_pairs()[i][:2], rounding_pairs()[i][2]["numpy"], 2 + i % 2)
    out["duplicates"] = lambda: {k: duplicates_case()[k] for k in ("points", "scores", "num", "radius")}
    out["long pass count"] = long_pass_case
    return out


PICK_NAMES = tuple(pick_builders())
_TRACES = {}


def traced(name):
    """(case, picked indices, trace) of a pick case, computed once per process"""
    if name not in _TRACES:
        c = pick_builders()[name]()
        _TRACES[name] = (c,) + greedy_trace(c["points"], c["scores"], c["num"], c["radius"])
    return _TRACES[name]
