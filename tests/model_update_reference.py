"""Cases, float64 restatements, bounds and wrong models for the stage that rewrites the model between frames: the densify / clone /
split / prune compaction, the key-frame append, the one-launch Adam step and the isotropic regulariser (csrc/densify.hip), the window
statistics (csrc/activations.hip) and their wrappers splatloc_amd/densify.py, optim.py, losses.isotropic_loss.  No GPU import.

  tests/golden/make_golden_model_update_edges.py   runs the reference's own GaussianModel.densify_and_prune / extend_from_pcd on the
                                                   densify and append cases below (tests/golden/model_update_edges.npz); inputs are NOT
                                                   stored: the builders are seeded and the fixture holds a checksum of every case's inputs
  tests/test_host_model_update_edges.py            fixture against the restatements, every case reaches its edge, every wrong model fails
  tests/test_gpu_model_update_edges.py             the device entry points against the restatements, within the bounds below

The builders use only IEEE float32 / float64 arithmetic on np.random.RandomState uniforms (no libm call), so they reproduce bit for bit.
Quantities a kernel passes through expf / logf sit either exactly where every implementation agrees (raw scale 0: exp = 1; raw opacity
0: sigmoid = 0.5) or at least MARGIN away from every threshold in the raw (log / logit) domain; the builders check that and redraw.

BOUNDS.  U = 2^-24 is the unit roundoff of float32, TINY = 2^-149 its smallest subnormal (absolute error of a rounding that underflows).
Each bound is a forward-error bound of the float32 expression against its float64 restatement FROM THE SAME float32 INPUTS: number of
roundings x U x the magnitudes of the terms they act on, plus the documented error of the device's libm (expf 1 ulp, logf 1 ulp, sinf /
cosf 2 ulp, sqrtf and division correctly rounded; 1 ulp <= 2 U relative).  A fused multiply-add removes roundings and adds none, so the
bounds hold for contracted and uncontracted code alike.

  split child scaling  y = log(exp(x) * (1 / 1.6f)):  exp 2U, the constant 1/1.6f 2U (1.6f and the division), the product U: a relative
      error of 5U inside the log is an absolute 5U of y; logf adds 2U |y| and the reference's `/ 1.6` form sits inside the same count.
      scaling_bound = 6U + 2U |y|.
  split child xyz  p + R(q/|q|) (z * exp(s)):  smp_k = z_k exp(s_k) carries 3U relative.  |q|^2 (4 products, 3 sums) 4U, sqrt and the
      division 2U more: every unit component 4U; a product of two 9U, the sum of two products 10U of at most 1, doubled exactly, the
      subtraction from 1 one more: every entry of R is good to 12U absolutely.  A row of R times smp: (12U + 3U + 3U) sum_k |smp_k|
      (entry error, smp error, the product and the two sums), the final sum U (|p| + sum |smp|).
      xyz_bound = 19U sum_k |smp_k| + U |p|, doubled (XYZ_SLACK) for the second-order terms the count drops.
  draws  z = sqrt(-2 log u0) cos(2 pi u1) from the SAME 24-bit uniforms:  log 2U, sqrt U + U: the radius 4U; the angle 2 pi f * u1 is
      off by at most 2U * 2 pi < 13U (the constant and the product), cosf / sinf 2 ulp = 4U: |dz| <= ra (4U + 13U + 4U).
      draw_bound = 21U ra (ra = the radius), + TINY.
  Adam (adam_element):  m' = m + (g - m) w1: 3 roundings on |m| + w1 |g - m|.  v' = v b2 + (w2 g) g: 4 roundings on b2 v + w2 g^2,
      each at least TINY (g ~ 1e-20 makes w2 g g subnormal).  The parameter is propagated, not counted:  s = sqrt(v') moves by at most
      min(dv / s, sqrt(dv)) + 2U s;  d = s c2 + eps by ds c2 + 4U d (the product, the sum, torch's division by the rounded sqrt(bc2));
      q = m' / d by (dm / d + |m'| dd / d^2)(1 + 2 dd / d) + U |q|;  p' = p - a q by a dq + 4U |a q| + U (|p| + |a q|)  (a = lr / bc1:
      torch rounds the double quotient of a double lr, adam_step that of the float lr: 2U of a q, the product and the difference 2 more).
  statistics:  accum += sqrt(gx^2 + gy^2) per seeing view: the norm 4U (two products, the sum, the root), the running sum U each time.
  isotropic:  t = mean_k(s) / (0.02 (1 - mk)):  SC - 1 sums, the division by SC, 0.02f, the difference, the product, the reciprocal, the
      final product: (SC + 5) U t; x = t - 1 adds U |x|.  The loss is a double sum rounded once: mean(dx) + U loss.  A row's gradient
      sign(x) / (SC 0.02 (1 - mk) count) passes 8 roundings: 8U of itself (the builders keep |x| away from its own bound: no sign flips).
"""
import hashlib
import zlib

import numpy as np

from oracle import densify as OD

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -149
GROUPS = OD.GROUPS
MARGIN = 0.02                 # raw-domain distance of every generic scale / opacity from every threshold
REDRAW_CAP = 16
XYZ_SLACK = 2.0
LN_1_6 = 0.47000362924573563
MAX_GRAD = 0.000244140625     # 2^-12: float32-exact, so accum / denom can equal it exactly
MARKER_THR = F32(0.005)
MAX_WINDOW_VIEWS = 8
ADAM_QUAD_CAP = 4096 * 256    # quads of adam_quad_kernel's first grid pass; elements of adam_kernel's
ISO_ROW_CAP = 1024 * 256      # rows of isotropic_fwd_kernel's first grid pass
ISO_BLOCK = 256

# (percent_dense, extent, ln(size_split), ln(size_prune)): the logs are literals so that the builders call no libm; the host test
# checks them against np.log of the thresholds
HYPERS = {
    "tie": (0.01, 100.0, 0.0, 2.302585092994046),                       # size_split = 1.0, size_prune = 10.0
    "below": (0.008, 124.99999237060547, 0.0, 2.5257285514665736),      # f32(double product) = 1 - 2^-24, float product = 1.0
    "above": (0.01, 100.00000762939453, 0.0, 2.302585169287991),        # f32(double product) = 1 + 2^-23, float product = 1.0
    "tenth": (0.01, 1.100000023841858, -4.509860006183766, -2.207274913189721),   # f32(0.1 * extent) != 0.1f * extent
}


def _seed(name):
    return zlib.crc32(name.encode())


def _noise(rs, shape):
    """unit-variance bell-shaped noise without libm: an Irwin-Hall sum of four uniforms"""
    return ((rs.rand(4, *shape).sum(axis=0) - 2.0) * 1.7320508075688772).astype(F32)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest()[:16], dtype=np.uint8).copy()


def exceeds(dev, bound):
    """True where a deviation is NOT within the bound (NaN and inf exceed every bound)"""
    return ~(np.asarray(dev) <= np.asarray(bound))


def worst_ratio(got, want, bound):
    """max |got - want| / bound; inf where a value is not finite or the bound is 0 and the values differ"""
    dev = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
    bound = np.broadcast_to(np.asarray(bound, F64), dev.shape)
    if dev.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == 0, 0.0, dev / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


def thresholds(percent_dense, extent):
    """(size_split, size_prune) as the reference forms them: the float32 rounding of the DOUBLE products"""
    return F32(percent_dense * extent), F32(0.1 * extent)


def thresholds_float_products(percent_dense, extent):
    """WRONG MODEL `float_products`: the float32 products of the float32 arguments"""
    return F32(F32(percent_dense) * F32(extent)), F32(F32(0.1) * F32(extent))


# =================================================================================================================================
# densify
# =================================================================================================================================
WIDTH_CASES = (  # P, scaling width, f_rest width, kp width, moments
    (1, 3, 0, 1, True), (2, 1, 9, 2, False), (255, 3, 45, 2, True), (256, 1, 0, 1, False), (257, 3, 9, 1, True),
    (257, 1, 45, 2, True), (1025, 1, 45, 1, False), (1025, 3, 0, 2, True), (1025, 3, 9, 1, True))
TIE_CASES = ("tie grad", "tie scale below", "tie scale at", "tie scale above", "tie opacity below", "tie opacity at",
             "tie opacity above", "tie marker", "products tenth")
OUTCOME_CASES = ("outcome none", "outcome all cloned", "outcome all split kept", "outcome all split pruned", "outcome all pruned",
                 "outcome parent size", "outcome key primitives")


def width_name(spec):
    return "widths P%d sc%d fr%d kp%d %s" % (spec[0], spec[1], spec[2], spec[3], "moments" if spec[4] else "bare")


def densify_case_names():
    return [width_name(s) for s in WIDTH_CASES] + list(TIE_CASES) + list(OUTCOME_CASES)


def _generic_raw(rs, shape, lo, hi, avoid):
    """uniform in [lo, hi), at least MARGIN from every value of `avoid`; (values, redraws used)"""
    x = (lo + (hi - lo) * rs.rand(*shape)).astype(F32)
    for n in range(REDRAW_CAP + 1):
        bad = np.zeros(shape, bool)
        for a in avoid:
            bad |= np.abs(x.astype(F64) - a) < MARGIN
        if not bad.any():
            return x, n
        x = np.where(bad, (lo + (hi - lo) * rs.rand(*shape)).astype(F32), x)
    raise AssertionError("redraw cap exceeded")


def _base_model(rs, P, SC, FR, KP, moments, hyper):
    """a generic model: every branch of the flag kernel taken, nothing through exp within MARGIN of a threshold"""
    _, _, ln_split, ln_prune = HYPERS[hyper]
    avoid = (ln_split, ln_prune, ln_prune + LN_1_6)
    sc, n1 = _generic_raw(rs, (P, SC), ln_split - 1.5, ln_prune + LN_1_6 + 0.6, avoid)
    op, n2 = _generic_raw(rs, (P, 1), -3.0, 3.0, (0.0,))
    rot = _noise(rs, (P, 4))
    rot[:, 0] = (F32(1.5) + rot[:, 0] * F32(0.25)).astype(F32)                      # |q| stays well above 0; stored un-normalised
    par = dict(xyz=(_noise(rs, (P, 3)) * F32(2)).astype(F32), f_dc=rs.rand(P, 1, 3).astype(F32),
               f_rest=rs.rand(P, FR // 3, 3).astype(F32), opacity=op,
               marker=((rs.rand(P, 1) < 0.3) * (0.01 + 0.89 * rs.rand(P, 1))).astype(F32), kp_score=rs.rand(P, KP).astype(F32),
               scaling=sc, rotation=rot)
    u = rs.rand(3, P, 1)
    accum = (rs.rand(P, 1) * (2.0 * MAX_GRAD)).astype(F32)
    accum = np.where(u[0] < 0.1, -accum, accum).astype(F32)                         # a negative sum: |g| clones, g itself never splits
    accum = np.where(u[1] < 0.15, F32(0), accum).astype(F32)
    denom = np.floor(u[2] * 4.0).astype(F32)                                        # 0: NaN (cold) with accum 0, +-inf otherwise
    m = v = None
    if moments:
        m = {k: _noise(rs, par[k].shape) for k in GROUPS if k != "marker"}
        v = {k: rs.rand(*par[k].shape).astype(F32) for k in GROUPS if k != "marker"}
    return dict(params=par, m=m, v=v, accum=accum, denom=denom, unit_noise=_noise(rs, (2, P, 3)), redraws=max(n1, n2))


def _plant(c, row, **kw):
    for k, val in kw.items():
        tgt = c[k] if k in ("accum", "denom") else c["params"][k]
        tgt[row] = np.asarray(val, F32)


def densify_case(name):
    """dict(name, params, m, v (dicts or None), accum, denom, unit_noise, hyper = the keyword arguments of the entry points, step,
    redraws, rows = {label: row} of the planted rows)"""
    rs = np.random.RandomState(_seed("densify " + name))
    hyper, min_opacity, screen, reg, rows = "tie", 0.5, 20.0, False, {}
    if name.startswith("widths "):
        spec = [s for s in WIDTH_CASES if width_name(s) == name][0]
        P, SC, FR, KP, mom = spec
        reg = bool(P % 2)
        c = _base_model(rs, P, SC, FR, KP, mom, hyper)
        if P == 1:                                         # a hot small row: cloned (the reference's squeeze() needs two rows left)
            _plant(c, 0, accum=[2 * MAX_GRAD], denom=[1], scaling=[-1, -1.5, -1.25], opacity=[2], marker=[0])
    elif name.startswith("tie ") or name.startswith("products "):
        P, SC = 257, 3
        lo, hi = [-1.0] * 3, [1.0] * 3                     # raw scales of a small (clone) and a large (split) Gaussian
        if name.startswith("tie scale"):
            hyper = name.split()[-1] if name.split()[-1] != "at" else "tie"
        if name == "products tenth":
            hyper = "tenth"
        if name.startswith("tie opacity"):
            min_opacity = float({"below": below(0.5), "at": F32(0.5), "above": above(0.5)}[name.split()[-1]])
        reg = name == "tie marker"
        c = _base_model(rs, P, SC, 9, 2, True, hyper)
        hot, cold = dict(accum=[2 * MAX_GRAD], denom=[1]), dict(accum=[0], denom=[1])
        plant = []
        if name == "tie grad":
            g = F32(MAX_GRAD)
            for lab, a, d in (("quotient", 3 * g, 3), ("at", g, 1), ("below", below(g), 1), ("above", above(g), 1), ("neg at", -g, 1),
                              ("neg below", -below(g), 1), ("nan", 0, 0), ("inf", g, 0), ("neg inf", -g, 0), ("neg zero", -0.0, 1)):
                for sz, raw in (("small", lo), ("large", hi)):
                    plant.append((f"{lab} {sz}", dict(accum=[a], denom=[d], scaling=raw, opacity=[2], marker=[0])))
        elif name.startswith("tie scale"):
            for lab, raw in (("all", [0, 0, 0]), ("first", [0, -1, -1]), ("last", [-1, -0.5, 0])):
                plant.append((f"hot {lab}", dict(scaling=raw, opacity=[2], marker=[0], **hot)))
                plant.append((f"cold {lab}", dict(scaling=raw, opacity=[2], marker=[0], **cold)))
        elif name.startswith("tie opacity"):
            for lab, raw, gr in (("cold", lo, cold), ("clone", lo, hot), ("split", hi, hot)):
                plant.append((lab, dict(scaling=raw, opacity=[0], marker=[0], **gr)))
        elif name == "tie marker":
            for lab, mk in (("at", MARKER_THR), ("below", below(MARKER_THR)), ("above", above(MARKER_THR)), ("zero", 0), ("key", 0.5)):
                for kind, raw, gr in (("cold", lo, cold), ("clone", lo, hot), ("split", hi, hot)):
                    plant.append((f"{lab} {kind}", dict(scaling=raw, opacity=[-2], marker=[mk], **gr)))
        # planted rows from row 0, and again so that they end on the last rows (a second and a third block of the flag kernel)
        for i, (lab, kw) in enumerate(plant):
            _plant(c, i, **kw)
            _plant(c, P - len(plant) + i, **kw)
            rows[lab] = i
            rows[lab + " (end)"] = P - len(plant) + i
    elif name.startswith("outcome "):
        P, SC = 6, 3
        c = _base_model(rs, P, SC, 9, 1, True, hyper)
        what = name[len("outcome "):]
        hot, cold = dict(accum=[2 * MAX_GRAD], denom=[1]), dict(accum=[0], denom=[1])
        small, large = [-1.0, -1.5, -2.0], [1.0, 0.5, 1.5]
        screen = 0.0
        for i in range(P):
            if what == "none":
                _plant(c, i, scaling=large if i % 2 else small, opacity=[2], **cold)
            elif what == "all cloned":
                _plant(c, i, scaling=small, opacity=[2], **hot)
            elif what == "all split kept":
                _plant(c, i, scaling=large, opacity=[2], **hot)
            elif what == "all split pruned":
                _plant(c, i, scaling=large, opacity=[-2], marker=[0], **hot)
            elif what == "all pruned":
                _plant(c, i, scaling=large if i % 2 else small, opacity=[-2], marker=[0], **cold)
            elif what == "key primitives":
                _plant(c, i, scaling=large if i % 2 else small, opacity=[-2], marker=[0.5 if i < 4 else 0], **(hot if i in (1, 2) else cold))
        if what == "key primitives":
            reg = True
        if what == "parent size":
            # size_prune = 10: ln 12 (1.2 over; children at 7.5, 0.75 under), ln 19.2 (children at 12), ln 7.5
            screen = 20.0
            ln12, ln19, ln75 = 2.4849066497880004, 2.954910279033736, 2.0149030205422647
            for i, (lab, raw, gr) in enumerate((("hot over", ln12, hot), ("cold over", ln12, cold), ("hot far over", ln19, hot),
                                               ("cold under", ln75, cold), ("hot under", ln75, hot), ("cold small", -1.0, cold))):
                _plant(c, i, scaling=[raw, -1.0, 0.5], opacity=[2], marker=[0], **gr)
                rows[lab] = i
    else:
        raise KeyError(name)
    pd, extent, _, _ = HYPERS[hyper]
    c.update(name=name, rows=rows, step=7.0, hyper_name=hyper,
             hyper=dict(max_grad=MAX_GRAD, min_opacity=min_opacity, extent=extent, max_screen_size=screen, percent_dense=pd,
                        primitive_reg=reg))
    return c


def densify_inputs(c):
    """every input array of a densify case, in a fixed order (for the fixture's checksum)"""
    out = [c["params"][k] for k in GROUPS] + [c["accum"], c["denom"], c["unit_noise"]]
    if c["m"] is not None:
        out += [c["m"][k] for k in GROUPS if k in c["m"]] + [c["v"][k] for k in GROUPS if k in c["v"]]
    h = c["hyper"]
    out.append(np.array([h["max_grad"], h["min_opacity"], h["extent"], h["max_screen_size"], h["percent_dense"],
                         float(h["primitive_reg"])], F64))
    return out


def densify_margin_ok(c):
    """the stated margin: every raw scale is 0 or MARGIN from ln(size_split), ln(size_prune) and the children's ln(1.6 size_prune);
    every raw opacity is 0 or MARGIN from logit(min_opacity) = 0 (min_opacity is 0.5 or its neighbours)"""
    _, _, ln_split, ln_prune = HYPERS[c["hyper_name"]]
    sc, op = c["params"]["scaling"].astype(F64), c["params"]["opacity"].astype(F64)
    ok = np.ones(sc.shape, bool)
    for a in (ln_split, ln_prune, ln_prune + LN_1_6):
        ok &= (np.abs(sc - a) >= MARGIN) | (sc == 0)
    return bool(ok.all()) and bool(((np.abs(op) >= MARGIN) | (op == 0)).all())


def densify_oracle(c):
    """oracle/densify.py on the case: (params, state or {}, source_row, source_kind)"""
    state = {} if c["m"] is None else {k: dict(m=c["m"][k], v=c["v"][k], step=c["step"]) for k in c["m"]}
    h = c["hyper"]
    return OD.densify_and_prune(c["params"], state, c["accum"], c["denom"], c["unit_noise"], h["max_grad"], h["min_opacity"],
                                h["extent"], h["max_screen_size"], h["percent_dense"], h["primitive_reg"])


DENSIFY_WRONG = ("grad_gt", "size_lt", "opacity_le", "float_products", "child_parent_size", "marker_lt", "split_abs_grad")


def densify_plan_model(c, wrong=None):
    """(source_row, source_kind) from the rules alone, written on the four sections of the flag kernel, independently of
    oracle/densify.py's sequence of concatenations.  `wrong`: one of DENSIFY_WRONG."""
    h = c["hyper"]
    P = c["accum"].shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (c["accum"][:, 0] / c["denom"][:, 0]).astype(F32)
        g = np.where(np.isnan(g), F32(0), g)
        s = np.exp(c["params"]["scaling"]).astype(F32)
        child = np.exp(np.log(s / F32(1.6)).astype(F32)).astype(F32).max(axis=1)
        op = (1.0 / (1.0 + np.exp(-c["params"]["opacity"][:, 0]))).astype(F32)
    smax = s.max(axis=1)
    thr = thresholds_float_products if wrong == "float_products" else thresholds
    size_split, size_prune = thr(h["percent_dense"], h["extent"])
    mg = F32(h["max_grad"])
    hot_c = (np.abs(g) > mg) if wrong == "grad_gt" else (np.abs(g) >= mg)
    hot_s = (g > mg) if wrong == "grad_gt" else ((np.abs(g) >= mg) if wrong == "split_abs_grad" else (g >= mg))
    small = (smax < size_split) if wrong == "size_lt" else (smax <= size_split)
    clone, split = hot_c & small, hot_s & ~(smax <= size_split)
    low = (op <= F32(h["min_opacity"])) if wrong == "opacity_le" else (op < F32(h["min_opacity"]))
    mk = c["params"]["marker"][:, 0]
    gate = np.ones(P, bool) if not h["primitive_reg"] else ((mk < MARKER_THR) if wrong == "marker_lt" else (mk <= MARKER_THR))
    use = bool(h["max_screen_size"])
    prune_self = (low | (use & (smax > size_prune))) & gate
    prune_child = (low | (use & ((smax if wrong == "child_parent_size" else child) > size_prune))) & gate
    keep = [~split & ~prune_self, clone & ~prune_self, split & ~prune_child, split & ~prune_child]
    src = np.concatenate([np.nonzero(k)[0] for k in keep])
    kind = np.concatenate([np.full(int(k.sum()), i, np.int64) for i, k in enumerate(keep)])
    return src, kind


def densify_split_f64(c, src, kind, unit_noise=None):
    """float64 twin of the split children's xyz and scaling for the rows (src, kind), from the same float32 inputs, and their bounds:
    (xyz64, xyz_bound, scaling64, scaling_bound) over ALL rows; rows that are copies hold the copy and bound 0"""
    par = {k: np.asarray(c["params"][k], F64) for k in ("xyz", "scaling", "rotation")}
    noise = np.asarray(c["unit_noise"] if unit_noise is None else unit_noise, F64)
    xyz, sc = par["xyz"][src].copy(), par["scaling"][src].copy()
    xb, sb = np.zeros_like(xyz), np.zeros_like(sc)
    ch = kind >= 2
    i = src[ch]
    z = noise[kind[ch] - 2, i]
    e = np.exp(par["scaling"][i])
    smp = z * (e if e.shape[1] == 3 else np.repeat(e, 3, axis=1))
    q = par["rotation"][i]
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                  2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                  2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    xyz[ch] = np.einsum("nij,nj->ni", R, smp) + par["xyz"][i]
    xb[ch] = XYZ_SLACK * (19 * U * np.abs(smp).sum(axis=1, keepdims=True) + U * np.abs(par["xyz"][i]))
    sc[ch] = par["scaling"][i] - LN_1_6
    sb[ch] = 6 * U + 2 * U * np.abs(sc[ch])
    return xyz, xb, sc, sb


def densify_values_wrong(c, out_p, out_state, src, kind, wrong):
    """WRONG MODELS of the values: `clone_moments` (clones inherit the source's moments), `child_scale` (children keep the parent's
    scale).  Returns modified copies of (params, state)."""
    p = {k: v.copy() for k, v in out_p.items()}
    st = {k: dict(m=v["m"].copy(), v=v["v"].copy(), step=v["step"]) for k, v in out_state.items()}
    if wrong == "clone_moments":
        for k in st:
            st[k]["m"][kind == 1] = c["m"][k][src[kind == 1]]
            st[k]["v"][kind == 1] = c["v"][k][src[kind == 1]]
    elif wrong == "child_scale":
        p["scaling"][kind >= 2] = c["params"]["scaling"][src[kind >= 2]]
    else:
        raise KeyError(wrong)
    return p, st


# =================================================================================================================================
# key-frame append
# =================================================================================================================================
APPEND_CASES = (  # P, N, scaling width, f_rest width, kp width, state
    (0, 5, 3, 9, 1, True), (0, 5, 1, 0, 2, False), (5, 0, 3, 45, 2, True), (1, 1, 1, 9, 1, False), (1, 1, 3, 0, 1, True),
    (255, 2, 3, 45, 1, True), (255, 2, 1, 0, 2, False), (256, 257, 1, 9, 2, True), (256, 257, 3, 45, 1, False))


def append_name(spec):
    return "append P%d N%d sc%d fr%d kp%d %s" % (spec[0], spec[1], spec[2], spec[3], spec[4], "state" if spec[5] else "bare")


def append_case_names():
    return [append_name(s) for s in APPEND_CASES]


def append_case(name):
    """dict(params, m, v (or None), extra = the N new rows by group, features [N,3,K] as extend_from_pcd takes them, step)"""
    spec = [s for s in APPEND_CASES if append_name(s) == name][0]
    P, N, SC, FR, KP, state = spec
    rs = np.random.RandomState(_seed(name))
    shapes = dict(xyz=(3,), f_dc=(1, 3), f_rest=(FR // 3, 3), opacity=(1,), marker=(1,), kp_score=(KP,), scaling=(SC,), rotation=(4,))
    par = {k: _noise(rs, (P,) + shapes[k]) for k in GROUPS}
    extra = {k: _noise(rs, (N,) + shapes[k]) for k in GROUPS}
    m = v = None
    if state:
        m = {k: _noise(rs, par[k].shape) for k in GROUPS if k != "marker"}
        v = {k: rs.rand(*par[k].shape).astype(F32) for k in GROUPS if k != "marker"}
    features = np.ascontiguousarray(np.concatenate((extra["f_dc"], extra["f_rest"]), axis=1).transpose(0, 2, 1))
    return dict(name=name, P=P, N=N, params=par, extra=extra, m=m, v=v, features=features, step=5.0)


def append_inputs(c):
    out = [c["params"][k] for k in GROUPS] + [c["extra"][k] for k in GROUPS]
    if c["m"] is not None:
        out += [c["m"][k] for k in GROUPS if k in c["m"]] + [c["v"][k] for k in GROUPS if k in c["v"]]
    return out


def append_expected(c):
    """(params, m, v): the rows appended, zero moments for the new rows (cat_tensors_to_optimizer)"""
    p = {k: np.concatenate((c["params"][k], c["extra"][k]), 0) for k in GROUPS}
    if c["m"] is None:
        return p, None, None
    m = {k: np.concatenate((c["m"][k], np.zeros_like(c["extra"][k])), 0) for k in c["m"]}
    v = {k: np.concatenate((c["v"][k], np.zeros_like(c["extra"][k])), 0) for k in c["v"]}
    return p, m, v


def outputs_checksum(params, m, v):
    """one checksum over the exactly-copied groups (all but xyz and scaling, which the split recomputes) and the moments"""
    arrs = [np.asarray(params[k], F32) for k in GROUPS if k not in ("xyz", "scaling")]
    if m is not None:
        arrs += [np.asarray(m[k], F32) for k in GROUPS if k in m] + [np.asarray(v[k], F32) for k in GROUPS if k in v]
    return checksum(*arrs)


# =================================================================================================================================
# Philox4x32-10 + Box-Muller (normal3 of densify.hip)
# =================================================================================================================================
DRAW_WORDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)
M32 = np.uint64(0xFFFFFFFF)


def philox4x32(seed, ctr_lo, ctr_hi, wrong=None):
    """ctr_lo: uint64 array (low counter words (row, copy)); seed, ctr_hi: Python ints below 2^64.  uint32 [n, 4].
    `wrong`: `no_k1` (the key's high word dropped), `no_ctr_hi` (the counter's high word dropped)."""
    ctr_lo = np.asarray(ctr_lo, np.uint64)
    c = [ctr_lo & M32, ctr_lo >> np.uint64(32), np.full(ctr_lo.shape, ctr_hi & 0xFFFFFFFF, np.uint64),
         np.full(ctr_lo.shape, 0 if wrong == "no_ctr_hi" else (ctr_hi >> 32), np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, 0 if wrong == "no_k1" else (seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def normal3(seed, draw_id, rows, copy, wrong=None):
    """(z [n,3] float64, bound [n,3]): the draws of normal3 for the source rows `rows` and one `copy`, evaluated in float64 from the same
    24-bit float32 uniforms and with the same pairing (z0, z1 from words 0, 1; z2 from words 2, 3)"""
    rows = np.asarray(rows, np.uint64)
    r = philox4x32(seed, (np.uint64(copy) << np.uint64(32)) | rows, draw_id, wrong)
    hi = (r >> np.uint32(8)).astype(F32)
    scale = F32(1.0 / 16777216.0)
    u0, u1 = ((hi[:, 0] + F32(0.5)) * scale).astype(F64), (hi[:, 1] * scale).astype(F64)
    u2, u3 = ((hi[:, 2] + F32(0.5)) * scale).astype(F64), (hi[:, 3] * scale).astype(F64)
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    z = np.stack([ra * np.cos(2 * np.pi * u1), ra * np.sin(2 * np.pi * u1), rb * np.cos(2 * np.pi * u3)], axis=1)
    bound = 21 * U * np.stack([ra, ra, rb], axis=1) + TINY
    return z, bound


def draws_case(P=257):
    """every row hot and large, nothing pruned, identity rotation, unit scales, parents at the origin: children's xyz = the draws"""
    par = dict(xyz=np.zeros((P, 3), F32), f_dc=np.zeros((P, 1, 3), F32), f_rest=np.zeros((P, 0, 3), F32),
               opacity=np.full((P, 1), 3, F32), marker=np.zeros((P, 1), F32), kp_score=np.zeros((P, 1), F32),
               scaling=np.zeros((P, 3), F32), rotation=np.tile(np.array([1, 0, 0, 0], F32), (P, 1)))
    # size_split = f32(0.001 * 100) = 0.1 < exp(0) = 1: split; min_opacity 0.005 << sigmoid(3); no size prune
    return dict(params=par, accum=np.ones((P, 1), F32), denom=np.ones((P, 1), F32),
                hyper=dict(max_grad=MAX_GRAD, min_opacity=0.005, extent=100.0, max_screen_size=0, percent_dense=0.001,
                           primitive_reg=False))


# =================================================================================================================================
# Adam
# =================================================================================================================================
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
TRAINING_LRS = dict(xyz=0.0016 * 6.0, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, marker=0.05, kp_score=0.05,
                    scaling=0.001 * 6.0, rotation=0.001)
MAGNITUDES = ("ordinary", "zero", "eps", "subnormal", "mixed")
STEPS = (1, 2, 1000, 30000)
GATE_THR = 0.005
STRIDE_RADII = 1031


def adam_case_names():
    return ([f"model P{P}" for P in (1, 2, 3, 5)] + ["widths"] + [f"{m} step {s}" for m in MAGNITUDES for s in STEPS]
            + ["gate", "gate nan only"])


def _adam_group(rs, name, shape, lr, magnitude, step, grad=True):
    p = _noise(rs, shape)
    n = _noise(rs, shape)
    if magnitude == "ordinary":
        g = (n * F32(1e-3)).astype(F32)
    elif magnitude == "zero":
        g = np.zeros(shape, F32)
    elif magnitude == "eps":            # 1e-13 .. 1e-16: sqrt(v) / sqrt(bc2) ~ eps = 1e-15
        g = (n * np.where(rs.rand(*shape) < 0.5, F32(1e-13), F32(1e-16))).astype(F32)
    elif magnitude == "subnormal":      # 1e-19 .. 1e-20: (1 - beta2) g^2 ~ 1e-41 .. 1e-43 is a float32 subnormal
        g = (n * np.where(rs.rand(*shape) < 0.5, F32(1e-19), F32(1e-20))).astype(F32)
    elif magnitude == "mixed":
        g = (n * F32(1e-3)).astype(F32)
    else:
        raise KeyError(magnitude)
    grp = dict(name=name, p=p, g=g if grad else None, m=None, v=None, step_prev=None, lr=lr)
    if step > 1:                        # carried-in moments of the magnitude the gradients would have left
        scale = {"ordinary": 1e-3, "zero": 1e-3, "eps": 1e-14, "subnormal": 1e-20, "mixed": 1.0}[magnitude]
        grp["m"] = (_noise(rs, shape) * F32(scale)).astype(F32)
        # second moments of the gradients' scale squared; 1e-40 is a float32 subnormal
        grp["v"] = (rs.rand(*shape) * (1e-40 if magnitude == "subnormal" else scale * scale)).astype(F32)
        grp["step_prev"] = float(step - 1)
    return grp


def adam_case(name):
    """dict(name, groups = [dict(name, p, g (None: no gradient), m, v, step_prev (None: no state yet), lr)], gate = (values [P,1],
    threshold, group name) or None).  One step() is the case."""
    rs = np.random.RandomState(_seed("adam " + name))
    gate = None
    if name.startswith("model P"):
        P = int(name[len("model P"):])
        shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 0, 3), opacity=(P, 1), marker=(P, 1), kp_score=(P, 1), scaling=(P, 3),
                      rotation=(P, 4))
        # the marker never has a gradient in map(), so it never has state either
        groups = [_adam_group(rs, k, shapes[k], TRAINING_LRS[k], "ordinary", 1 if (P % 2 or k == "marker") else 3, grad=k != "marker")
                  for k in GROUPS]
        gate = ((rs.rand(P, 1) < 0.5).astype(F32) * F32(0.5), GATE_THR, "xyz")
    elif name == "widths":
        P = 7
        groups = [_adam_group(rs, f"w{w}", (P, w), 1e-2 / (i + 1), "ordinary", 2, grad=(i != 2))
                  for i, w in enumerate((1, 3, 5, 4, 9))]
    elif name.startswith("gate"):
        P = 12
        thr = F32(GATE_THR)
        vals = [thr, above(thr), below(thr), np.nan, 0.0, 0.5, -1.0, np.inf, thr, np.nan, above(thr), below(thr)]
        if name == "gate nan only":
            vals = [np.nan] * P
        groups = [_adam_group(rs, "xyz", (P, 3), 1e-2, "ordinary", 2), _adam_group(rs, "opacity", (P, 1), 5e-2, "ordinary", 2)]
        gate = (np.array(vals, F32).reshape(P, 1), GATE_THR, "xyz")
    else:
        mag, _, step = name.rpartition(" step ")
        groups = [_adam_group(rs, "xyz", (37, 3), 1e-2, mag, int(step)), _adam_group(rs, "opacity", (37, 1), 5e-2, mag, int(step))]
    return dict(name=name, groups=groups, gate=gate)


def adam_stride_case(kind):
    """`quads`: one [1398103, 3] group = 1,048,577 full quads and a partial one, for the aligned kernel; `elements`: one group of
    1,048,577 elements for the scalar kernel.  Both with a radii tail of STRIDE_RADII entries behind them, in the second grid pass."""
    rs = np.random.RandomState(_seed("adam stride " + kind))
    shape = (1398103, 3) if kind == "quads" else (1048577, 1)
    grp = _adam_group(rs, "xyz", shape, 1e-2, "ordinary", 3)
    gate = ((rs.rand(shape[0], 1) < 0.3).astype(F32) * F32(0.5), GATE_THR, "xyz")
    radii = (np.floor(rs.rand(STRIDE_RADII) * 40) * (rs.rand(STRIDE_RADII) < 0.6) - (rs.rand(STRIDE_RADII) < 0.1)).astype(np.int32)
    max_radii = (rs.rand(STRIDE_RADII) * 30).astype(F32)
    return dict(name="stride " + kind, groups=[grp], gate=gate, radii=radii, max_radii=max_radii)


def radii_expected(radii, max_radii):
    return np.where(radii > 0, np.maximum(max_radii, radii.astype(F32)), max_radii).astype(F32)


ADAM_WRONG = ("eps_before_bc", "beta_for_omb", "gate_per_element")


def adam_f64(grp, gate=None, wrong=None):
    """One step of adam_element in float64 from the group's float32 inputs, with the host scalars formed as adam_step forms them.
    None for a skipped group (no gradient, or no elements): it gets no state.  Otherwise dict(p, m, v, step, bp, bm, bv): the
    float64 results and their bounds (module docstring)."""
    if grp["g"] is None or grp["p"].size == 0:
        return None
    p, g = grp["p"].astype(F64), grp["g"].astype(F64)
    m = np.zeros_like(p) if grp["m"] is None else grp["m"].astype(F64)
    v = np.zeros_like(p) if grp["v"] is None else grp["v"].astype(F64)
    step = 1.0 if grp["step_prev"] is None else grp["step_prev"] + 1.0
    if gate is not None and gate[2] == grp["name"]:
        vals, thr = np.asarray(gate[0], F32).reshape(-1), F32(gate[1])
        with np.errstate(invalid="ignore"):
            closed = vals > thr                                      # a NaN gate does not close it
        rows = p.shape[0]
        if wrong == "gate_per_element":
            mask = closed[np.arange(p.size) % rows].reshape(p.shape)
        else:
            mask = np.broadcast_to(closed.reshape((rows,) + (1,) * (p.ndim - 1)), p.shape)
        g = np.where(mask, 0.0, g)
    w1, w2, b2, eps = F64(F32(1.0 - BETA1)), F64(F32(1.0 - BETA2)), F64(F32(BETA2)), F64(F32(EPS))
    if wrong == "beta_for_omb":
        w1, w2 = F64(F32(BETA1)), F64(F32(BETA2))
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    a = F64(F32(F64(F32(grp["lr"])) / bc1))
    c2 = F64(F32(1.0 / np.sqrt(bc2)))
    m1 = m + (g - m) * w1
    v1 = v * b2 + (w2 * g) * g
    s = np.sqrt(v1)
    d = (s + eps) * c2 if wrong == "eps_before_bc" else s * c2 + eps
    q = m1 / d
    p1 = p - a * q
    bm = 3 * U * (np.abs(m) + w1 * np.abs(g - m)) + 3 * TINY
    bv = 4 * U * (b2 * v + w2 * g * g) + 4 * TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s > 0, np.minimum(bv / s, np.sqrt(bv)), np.sqrt(bv)) + 2 * U * s
    dd = ds * c2 + 4 * U * d
    dq = (bm / d + np.abs(m1) * dd / (d * d)) * (1 + 2 * dd / d) + U * np.abs(q)
    bp = a * dq + 4 * U * np.abs(a * q) + U * (np.abs(p) + np.abs(a * q))
    return dict(p=p1, m=m1, v=v1, step=step, bp=bp, bm=bm, bv=bv)


# =================================================================================================================================
# window statistics
# =================================================================================================================================
STATS_CASES = tuple((V, P, om) for V in (1, 2, 8, 9) for P in (1, 255, 257) for om in (False, True)) + ((9, 513, False),)


def stats_case(V, P, only_max):
    """radii [V,P] int32, grads [V,P,3], the three state vectors.  Row i is seen by the views of the bit pattern (i + 1) mod 2^V
    (P > 2^V: every subset); a view that does not see a row holds radius 0 or a negative one.  Rows no view sees start as NaN, -0.0
    and inf."""
    rs = np.random.RandomState(_seed(f"stats {V} {P} {only_max}"))
    pat = (np.arange(P) + 1) % (1 << V) if P > 1 else np.array([1 if V == 1 else 2])
    sees = ((pat[None, :] >> np.arange(V)[:, None]) & 1).astype(bool)
    pos = (1 + np.floor(rs.rand(V, P) * 60)).astype(np.int32)
    neg = -(np.floor(rs.rand(V, P) * 3)).astype(np.int32)                     # 0, -1, -2
    radii = np.where(sees, pos, neg).astype(np.int32)
    grads = (_noise(rs, (V, P, 3)) * F32(1e-3)).astype(F32)
    accum, denom = (rs.rand(P) * 1e-2).astype(F32), np.floor(rs.rand(P) * 5).astype(F32)
    max_radii = (rs.rand(P) * 40).astype(F32)
    unseen = np.nonzero(~sees.any(axis=0))[0]
    fill = np.array([np.nan, -0.0, np.inf], F32)
    for j, i in enumerate(unseen):
        accum[i], denom[i], max_radii[i] = fill[j % 3], fill[(j + 1) % 3], fill[(j + 2) % 3]
    return dict(V=V, P=P, only_max=only_max, radii=radii, grads=grads, accum=accum, denom=denom, max_radii=max_radii, sees=sees)


def stats_f64(c, wrong=None):
    """(accum64, accum_bound, denom, max_radii) after the window, in view order.  `wrong` = `count_unseen`: a view counts whatever its
    radius.  Rows no view sees are returned as they came (compare their bits)."""
    a, n, mx = c["accum"].astype(F64), c["denom"].copy(), c["max_radii"].copy()
    b = np.zeros_like(a)
    for vw in range(c["V"]):
        vis = c["radii"][vw] > 0 if wrong != "count_unseen" else np.ones(c["P"], bool)
        g = c["grads"][vw].astype(F64)
        nrm = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
        a = np.where(vis, a + nrm, a)
        b = np.where(vis, b + 4 * U * nrm + U * np.abs(a), b)
        n = np.where(vis, n + F32(1), n).astype(F32)
        mx = np.where(vis, np.maximum(mx, c["radii"][vw].astype(F32)), mx).astype(F32)
    return a, b, n, mx


# =================================================================================================================================
# isotropic regulariser
# =================================================================================================================================
ISO_CASES = tuple((SC, P) for SC in (1, 3) for P in (0, 1, 5, 16385, 262145))


def iso_case(SC, P, empty=False):
    """activated scaling [P,SC], marker [P,1]: markers at MARKER_THR, its neighbours, 0, and far above; |x| kept >= 1e-3 (no sign tie)"""
    rs = np.random.RandomState(_seed(f"iso {SC} {P} {empty}"))
    planted = np.array([above(MARKER_THR), MARKER_THR, below(MARKER_THR), 0.0, 0.9], F32)
    mk = ((rs.rand(P, 1) < 0.4) * (0.01 + 0.85 * rs.rand(P, 1))).astype(F32)
    k = min(P, planted.size)
    mk[:k, 0] = planted[:k]
    if P >= 2 * planted.size:
        mk[-planted.size:, 0] = planted[::-1]
    if empty:
        mk = np.minimum(mk, MARKER_THR)
    # mean(s) = 0.02 (1 - mk) (1 + x), x in +-[0.05, 0.8]
    x = ((0.05 + 0.75 * rs.rand(P, 1)) * np.where(rs.rand(P, 1) < 0.5, -1.0, 1.0))
    mean = 0.02 * (1.0 - mk.astype(F64)) * (1.0 + x)
    r = rs.rand(P, SC)
    s = (mean * (1.0 + 0.8 * (r - r.mean(axis=1, keepdims=True)))).astype(F32)        # anisotropic columns, the same mean
    return dict(SC=SC, P=P, scaling=s, marker=mk)


def iso_f64(c, wrong=None):
    """(loss64, loss_bound, grad64 [P,SC], grad_bound, margin_ok).  `wrong` = `mask_ge`: marker >= 0.005 for >."""
    s, mk = c["scaling"].astype(F64), c["marker"].astype(F64)[:, 0]
    SC = c["SC"]
    mask = (c["marker"][:, 0] >= MARKER_THR) if wrong == "mask_ge" else (c["marker"][:, 0] > MARKER_THR)
    cnt = int(mask.sum())
    grad = np.zeros_like(s)
    if cnt == 0:
        return 0.0, 0.0, grad, np.zeros_like(s), True
    inv = 1.0 / (F64(F32(0.02)) * (1.0 - mk))
    t = s.mean(axis=1) * inv
    x = t - 1.0
    dx = (SC + 5) * U * np.abs(t) + U * np.abs(x)
    loss = float(np.abs(x[mask]).mean())
    lb = float(dx[mask].mean()) + U * loss
    grad[mask] = (np.sign(x[mask]) * inv[mask] / SC / cnt)[:, None]
    return loss, lb, grad, 8 * U * np.abs(grad), bool((np.abs(x[mask]) > 64 * dx[mask]).all())
