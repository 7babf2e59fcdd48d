"""References, bounds, models and named cases of the activation-stage edge tests (tests/test_gpu_activation_edges.py,
tests/test_host_activation_edges.py): activate_fwd_kernel / activate_bwd_kernel / densification_stats_kernel of
csrc/activations.hip and the arithmetic of csrc/activation_math.h.

* `reference`: a float64 restatement from torch CPU ops under autograd (torch.exp, torch.nn.functional.normalize, torch.sigmoid, the
  SH polynomials as a table of monomials, clamp_min, cat).  Nothing of oracle/activations.py's hand-derived backward is used.  Beside the
  values it returns, per output element, the sum of the absolute values of the terms that enter it (written out by hand: they
  scale the bars, they are not compared).
* Bars are elementwise: gamma(n) * sum|terms| (+ 2^-126 wherever the terms are not all zero: a result below the normal range may be
  flushed).  `roundings` states n per quantity.  Where the terms are all zero the device must hold an exact zero.
  - expf, sqrtf and `/`: the MEASURED way.  No accuracy statement of the device library is at hand (the compiler's help names
    -fhip-fp32-correctly-rounded-divide-sqrt without saying what holds when it is not given), so each counts as four times the worst
    relative error of torch's CPU float32 exp / sqrt / division against float64 on the values of the cases, in units of 2^-24
    (`measured_roundings`: about 4 for the root and the division, which the CPU rounds correctly, and a little more for exp).
  A ratio is never NaN: a NaN or infinity where the reference (rounded to float32) has none counts as infinite; where it has one the
  device must have the same.
* The exact family (`check_exact`): bit for bit against float32 numpy.
* `model32`: the two kernels in float32 numpy, quad by quad, with one deliberate defect per name of `WRONG`; `stats_model` likewise.
* Named, seeded cases (`CASES`), each with the edge it exists for.

Rows near the clamp: an element of `raw = eval_sh + 0.5` whose float64 value lies within the forward bar of 0 is `near`: float32
may decide the clamp either way.  The checks take the device's own decision (d_f_dc != 0: every case has nonzero upstream colour
gradients) and hold the gradients to the reference evaluated with THAT set of passing channels; away from `near` the decision itself must
be the reference's.  `near` rows are capped at 5 % of a case's rows (`near_rows`, asserted by the builders)."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-12
F32 = np.float32

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)

# basis function k of eval_sh as monomials (coefficient, (power of x, of y, of z))
SH_TABLE = (
    ((C0, (0, 0, 0)),),
    ((-C1, (0, 1, 0)),), ((C1, (0, 0, 1)),), ((-C1, (1, 0, 0)),),
    ((C2[0], (1, 1, 0)),), ((C2[1], (0, 1, 1)),),
    ((2 * C2[2], (0, 0, 2)), (-C2[2], (2, 0, 0)), (-C2[2], (0, 2, 0))),
    ((C2[3], (1, 0, 1)),), ((C2[4], (2, 0, 0)), (-C2[4], (0, 2, 0))),
    ((3 * C3[0], (2, 1, 0)), (-C3[0], (0, 3, 0))),
    ((C3[1], (1, 1, 1)),),
    ((4 * C3[2], (0, 1, 2)), (-C3[2], (2, 1, 0)), (-C3[2], (0, 3, 0))),
    ((2 * C3[3], (0, 0, 3)), (-3 * C3[3], (2, 0, 1)), (-3 * C3[3], (0, 2, 1))),
    ((4 * C3[4], (1, 0, 2)), (-C3[4], (3, 0, 0)), (-C3[4], (1, 2, 0))),
    ((C3[5], (2, 0, 1)), (-C3[5], (0, 2, 1))),
    ((C3[6], (3, 0, 0)), (-3 * C3[6], (1, 2, 0))),
)


def gamma(n):
    """n roundings of relative size 2^-24 each, compounded (Higham's gamma_n)"""
    return n * U / (1.0 - n * U)


def _mono(xyz, powers, lib):
    """x^a y^b z^c by repeated multiplication (no pow: its derivative at 0 stays a plain 0)"""
    out = lib.ones_like(xyz[0])
    for v, p in zip(xyz, powers):
        for _ in range(p):
            out = out * v
    return out


def eval_sh(deg, sh, dirs):
    """sum_k B_k(dir) sh[..., k] over the (deg + 1)^2 active coefficients: sh [P, 3, K] torch, dirs [P, 3] (unused at degree 0)"""
    result = C0 * sh[..., 0]
    if deg > 0:
        xyz = (dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3])
        for k in range(1, (deg + 1) ** 2):
            for coef, powers in SH_TABLE[k]:
                result = result + coef * _mono(xyz, powers, torch) * sh[..., k]
    return result


def _basis_abs(deg, d):
    """numpy float64: Babs [P, M] = sum |monomials| of B_k, dBabs [P, M, 3] likewise for dB_k/d(x, y, z)"""
    P, M = d.shape[0], (deg + 1) ** 2
    a = (np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2]))
    Babs, dBabs = np.zeros((P, M)), np.zeros((P, M, 3))
    for k in range(M):
        for coef, powers in SH_TABLE[k]:
            Babs[:, k] += abs(coef) * _mono(a, powers, np)
            for j in range(3):
                if powers[j]:
                    low = tuple(p - (i == j) for i, p in enumerate(powers))
                    dBabs[:, k, j] += abs(coef) * powers[j] * _mono(a, low, np)
    return Babs, dBabs


# ---- the roundings counted on the kernel's path, per quantity ----------------------------------------------------------------------
# E, S, D = measured_roundings(): what one expf, one sqrtf, one division may cost, in roundings; d = active degree, M = (d + 1)^2
#   scales      expf: E
#   rotations   ||q||^2: 4 products + 3 sums of positive terms = 7, halved by the root: 4; the root S; the division D: 4 + S + D
#   opacities   expf E, 1 + e: 1, the division D: E + 1 + D
#   a direction component (DIR): the difference 1; |v|^2: 5 roundings, halved: 3; the root S; the division D: 4 + S + D
#   colours     a monomial of degree <= d in the direction: d DIR; the polynomial's own operations <= 6; the sum over M terms: M;
#               + 0.5: 1
#   d_scaling   expf E, the product 1, the sum of the three upstream gradients at SC = 1: 2: E + 3
#   d_rotation  n: 4 + S; u = q / n: 4 + S + D; u . g: that + 7; u (u . g): the two + 1; the difference 1; / n: D + 4 + S:
#               3 S + 3 D + 21
#   d_opacity   s: E + 1 + D, in s and in 1 - s; the difference 1; two products: 2 (E + 1 + D) + 3, terms |g| s (1 + s)
#   d_f_dc      C0 g: 1 (taken as 2)
#   d_f_rest    B_k: d DIR + 6; the product 1
#   d_xyz       at degree 3: dB: 2 DIR + 6; w = sum_c sh_c g_c: 5; dB w: 1; the sum over 15 terms: 15; the dot with the direction:
#               DIR + 5; x (x . g): DIR + 1; the difference 1; / |v|: D + 3 + S: 4 DIR + S + D + 37, used at every degree
def roundings(deg):
    E, S, D = measured_roundings()
    M = (deg + 1) ** 2
    DIR = 4 + S + D
    return {"scales": E, "rotations": 4 + S + D, "opacities": E + 1 + D, "colors": deg * DIR + 6 + M + 1, "d_scaling": E + 3,
            "d_rotation": 3 * S + 3 * D + 21, "d_opacity": 2 * (E + 1 + D) + 3, "d_f_dc": 2, "d_f_rest": deg * DIR + 7,
            "d_xyz": 4 * DIR + S + D + 37, "d_extra": 0}


FORWARD = ("scales", "rotations", "opacities", "colors")
BACKWARD = ("d_xyz", "d_f_dc", "d_f_rest", "d_scaling", "d_rotation", "d_opacity", "d_extra")


@functools.lru_cache(maxsize=None)
def measured_roundings():
    """(E, S, D): four times the worst relative error of torch's CPU float32 exp, sqrt and division against float64, in units of
    2^-24, over the values the cases put through them: the exp arguments (log-scales, negated logits) with a normal float32 result,
    the squared norms of the quaternions and of the view vectors, and the quotients component / norm"""
    worst = [0.0, 0.0, 0.0]
    for name in CASES:
        c = case(name)
        x = np.concatenate([c["scaling"].ravel(), -c["opacity"].ravel()]).astype(F32)
        x = x[np.isfinite(x) & (x > -87.0) & (x < 88.0)]
        v = (c["xyz"] - c["campos"][None]).astype(F32)
        sq = np.concatenate([(c["rotation"].astype(F32) ** 2).sum(1), (v ** 2).sum(1)]).astype(F32)
        sq = sq[sq > F32(TINY)]
        num = np.concatenate([c["rotation"].astype(F32).ravel(), v.ravel()])
        den = np.sqrt(np.concatenate([np.repeat((c["rotation"].astype(F32) ** 2).sum(1), 4), np.repeat((v ** 2).sum(1), 3)])).astype(F32)
        keep = (den > F32(1e-18)) & (np.abs(num) > F32(1e-18))
        num, den = num[keep], den[keep]
        for i, (got, ref) in enumerate((
                (torch.exp(torch.from_numpy(x)), np.exp(x.astype(np.float64))),
                (torch.sqrt(torch.from_numpy(sq)), np.sqrt(sq.astype(np.float64))),
                (torch.from_numpy(num) / torch.from_numpy(den), num.astype(np.float64) / den.astype(np.float64)))):
            worst[i] = max(worst[i], float(np.max(np.abs(got.double().numpy() - ref) / np.abs(ref))))
    return tuple(4.0 * w / U for w in worst)


# ---- the float64 reference -------------------------------------------------------------------------------------------------------

INPUTS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "extra")


def reference(c, passing=None, dtype=np.float64):
    """float64 values and sums of |terms| of every output of the forward and the backward of case `c`.  `passing` [P, 3] bool: the
    clamp's decision per colour channel, given (rgb = raw where passing, 0 elsewhere) instead of taken by clamp_min.  `dtype`
    float32: the same torch ops in float32 (`torch32`); the terms and bars stay float64."""
    P, K, deg, SC, E = c["P"], c["K"], c["deg"], c["SC"], c["E"]
    M = (deg + 1) ** 2
    with np.errstate(all="ignore"):
        t = {k: torch.from_numpy(np.array(c[k], dtype)).requires_grad_(True) for k in INPUTS if c[k] is not None}
        campos = torch.from_numpy(np.asarray(c["campos"], dtype))
        scales = torch.exp(t["scaling"])
        if SC == 1:
            scales = scales.repeat(1, 3)
        rotations = torch.nn.functional.normalize(t["rotation"])
        opacities = torch.sigmoid(t["opacity"])
        feats = torch.cat((t["f_dc"], t["f_rest"]), dim=1)                      # [P, K, 3]
        shs_view = feats.transpose(1, 2)                                         # [P, 3, K]
        dirs = None
        if deg > 0:
            v = t["xyz"] - campos[None, :]
            dirs = v / v.norm(dim=1, keepdim=True)
        raw = eval_sh(deg, shs_view, dirs) + 0.5
        raw32 = None
        if deg == 0:      # the exact family: the decision is float32's own, fl(fl(C0 f) + 0.5) >= 0 (see `exact_expected`)
            raw32 = (F32(C0) * np.asarray(c["f_dc"], F32)[:, 0, :]).astype(F32) + F32(0.5)
            if passing is None:
                passing = raw32 >= 0
        if passing is None:
            rgb = torch.clamp_min(raw, 0.0)
            passing = (raw.detach() >= 0).numpy()
        else:
            passing = np.asarray(passing, bool)
            rgb = raw * torch.from_numpy(passing.astype(dtype))
        colors = torch.cat((rgb, t["extra"]), dim=1) if E else rgb
        G = {k: torch.from_numpy(np.asarray(c["G_" + k], dtype)) for k in FORWARD}
        ((scales * G["scales"]).sum() + (rotations * G["rotations"]).sum() + (opacities * G["opacities"]).sum()
         + (colors * G["colors"]).sum()).backward()
        grad = lambda k: np.zeros(t[k].shape) if t[k].grad is None else t[k].grad.numpy()  # noqa: E731
        ref = {"scales": scales.detach().numpy(), "rotations": rotations.detach().numpy(), "opacities": opacities.detach().numpy(),
               "colors": colors.detach().numpy(), "d_xyz": grad("xyz"), "d_f_dc": grad("f_dc"), "d_f_rest": grad("f_rest"),
               "d_scaling": grad("scaling"), "d_rotation": grad("rotation"), "d_opacity": grad("opacity"),
               "d_extra": grad("extra") if E else np.zeros((P, 0)), "raw": raw.detach().numpy(), "passing": passing}
        ref["raw_zero"] = (raw32 == 0) if deg == 0 else (ref["raw"] == 0)
        # ---- sums of |terms|
        g = {k: np.abs(np.asarray(c["G_" + k], np.float64)) for k in FORWARD}
        sc = np.exp(np.asarray(c["scaling"], np.float64))
        q = np.asarray(c["rotation"], np.float64)
        nrm = np.sqrt((q * q).sum(1, keepdims=True))
        n = np.maximum(nrm, EPS)
        s = 1.0 / (1.0 + np.exp(-np.asarray(c["opacity"], np.float64)))
        fa = np.abs(np.concatenate([np.asarray(c["f_dc"], np.float64), np.asarray(c["f_rest"], np.float64)], axis=1))   # [P, K, 3]
        if deg > 0:
            vv = np.asarray(c["xyz"], np.float64) - np.asarray(c["campos"], np.float64)[None]
            vlen = np.sqrt((vv * vv).sum(1, keepdims=True))
            d = vv / vlen
        else:
            vlen, d = np.ones((P, 1)), np.zeros((P, 3))
        Babs, dBabs = _basis_abs(deg, d)
        col_terms = np.einsum("pk,pkc->pc", Babs, fa[:, :M]) + 0.5
        gc = g["colors"][:, :3] * passing
        ua = np.abs(q) / n
        T = {"scales": np.repeat(sc, 3, axis=1) if SC == 1 else sc, "rotations": ua, "opacities": s,
             "colors": np.concatenate([col_terms, np.abs(np.asarray(c["extra"], np.float64))], axis=1) if E else col_terms,
             "d_scaling": (g["scales"] * sc).sum(1, keepdims=True) if SC == 1 else g["scales"] * sc,
             "d_rotation": np.where(nrm < EPS, g["rotations"] / EPS,
                                    (g["rotations"] + ua * (ua * g["rotations"]).sum(1, keepdims=True)) / n),
             "d_opacity": g["opacities"] * s * (1.0 + s),
             "d_f_dc": (C0 * gc)[:, None, :], "d_extra": g["colors"][:, 3:]}
        fr = np.zeros((P, K - 1, 3))
        fr[:, :M - 1] = Babs[:, 1:, None] * gc[:, None, :]
        T["d_f_rest"] = fr
        W = (fa[:, :M] * gc[:, None, :]).sum(2)                                   # [P, M]
        A = np.einsum("pkj,pk->pj", dBabs, W)
        T["d_xyz"] = (A + np.abs(d) * (np.abs(d) * A).sum(1, keepdims=True)) / vlen
        # a scale that overflows float32 is infinite in every float32 evaluation, and its gradient g * inf with it
        sc32 = sc.astype(F32).astype(np.float64)
        over = np.isinf(sc32).any(1)
        if over.any() and dtype is np.float64:
            gs = np.asarray(c["G_scales"], np.float64)          # (an isotropic scale: `repeat` sums its three gradients first)
            ref["d_scaling"][over] = ((gs.sum(1, keepdims=True) if SC == 1 else gs) * sc32)[over]
        N = roundings(deg)
        ref["bar"] = {k: gamma(N[k]) * T[k] + TINY * (T[k] > 0) for k in T}
        ref["terms"] = T
        ref["near"] = (np.abs(ref["raw"]) <= ref["bar"]["colors"][:, :3]) if deg > 0 else np.zeros((P, 3), bool)
    return ref


def torch32(c):
    """the restatement in float32 on the CPU, in the shape of a device run (what torch itself computes for the reference's model)"""
    r = reference(c, dtype=np.float32)
    out = {k: r[k] for k in FORWARD + BACKWARD}
    if c["deg"] == 0:
        out["d_xyz"] = None
    return out


def worst(got, ref, bar):
    """largest |got - ref| / bar.  Never NaN: where the float32 rounding of `ref` is infinite or NaN, `got` must be the same (ratio
    0, else infinite); elsewhere an error above a zero bar, a NaN or an infinity counts as infinite."""
    got, ref, bar = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bar, np.float64)
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r32 = ref.astype(F32).astype(np.float64)
        special = ~np.isfinite(r32)
        same = (np.isnan(r32) & np.isnan(got)) | (r32 == got)
        err = np.abs(got - ref)
        ok = err <= bar
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)
        ratio = np.where(ok | (np.isfinite(ratio) & (ratio > 1.0)), ratio, np.inf)
        ratio = np.where(special, np.where(same, 0.0, np.inf), ratio)
    return float(ratio.max())


def within(r):
    return all(v <= 1.0 for v in r.values())


def device_passing(out):
    """the clamp's decision as the backward took it in the colour quads"""
    return np.asarray(out["d_f_dc"])[:, 0, :] != 0


def check_bounded(run, name):
    """worst ratio per quantity of `run(case)` (a dict of float32 arrays by the names of FORWARD + BACKWARD; d_xyz may be None at degree
    0) on case `name`, plus `clamp`: infinite when the decision differs from the reference's away from the near rows"""
    c = case(name)
    out = run(c)
    ref = reference_of(name)
    r = {}
    pd = device_passing(out)
    differs = pd != ref["passing"]
    r["clamp"] = float("inf") if (differs & ~ref["near"]).any() else 0.0
    refb = reference(c, passing=pd) if differs.any() else ref
    for k in FORWARD:
        r[k] = worst(out[k], ref[k], ref["bar"][k])
    for k in BACKWARD:
        got = out[k]
        if k == "d_xyz" and got is None:
            assert c["deg"] == 0
            continue
        if k == "d_extra" and got is None:
            assert c["E"] == 0
            continue
        if k == "d_f_rest" and got is None:
            assert c["K"] == 1
            continue
        r[k] = worst(np.asarray(got).reshape(refb[k].shape), refb[k], refb["bar"][k])
    return r


def check_consistency(out, name):
    """the clamp's three decisions agree, on every row: failures by name"""
    c = case(name)
    ref = reference_of(name)
    pd = device_passing(out)
    rgb = np.asarray(out["colors"])[:, :3]
    failed = []
    if (~pd & (rgb != 0)).any():
        failed.append("a blocked channel with a nonzero colour")
    if ((rgb > 0) & ~pd).any():
        failed.append("a positive colour whose gradient is blocked")
    if (pd & (rgb == 0) & ~ref["near"] & ~ref["raw_zero"]).any():      # raw == +0 passes with a colour of 0
        failed.append("a passing channel with a zero colour away from the clamp")
    if out.get("d_f_rest") is not None and c["K"] > 1:
        fr = np.asarray(out["d_f_rest"]).reshape(c["P"], c["K"] - 1, 3)
        if (fr[np.broadcast_to(~pd[:, None, :], fr.shape)] != 0).any():
            failed.append("d_f_rest nonzero in a blocked channel")
    if c["deg"] > 0:
        dx = np.asarray(out["d_xyz"], np.float64)
        blocked = ~pd.any(1)
        if (dx[blocked] != 0).any():
            failed.append("d_xyz nonzero in a row whose three channels are blocked")
        refb = reference(c, passing=pd)
        if not worst(dx, refb["d_xyz"], refb["bar"]["d_xyz"]) <= 1.0:
            failed.append("d_xyz is not that of the passing channels of d_f_dc")
    return failed


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def same_bits(a, b, nan_payload=False):
    """float32 arrays equal bit for bit (`nan_payload`: any NaN equals any NaN)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    eq = _bits(a) == _bits(b)
    if nan_payload:
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(eq.all())


def exact_expected(c):
    """the float32 numpy model of the exact family of case `c`"""
    e = {}
    if c["E"]:
        e["extras"] = c["extra"]
        e["d_extra"] = np.ascontiguousarray(c["G_colors"][:, 3:])
    if c["deg"] == 0:
        raw = (F32(C0) * c["f_dc"][:, 0, :]).astype(F32) + F32(0.5)
        e["rgb"] = np.maximum(raw, F32(0))
        e["d_f_dc"] = np.where(raw >= 0, (F32(C0) * c["G_colors"][:, :3]).astype(F32), F32(0))[:, None, :]
    return e


def check_exact(out, name):
    """the exact family of `out` (run(case)) on case `name`: the names that are not bit for bit what float32 numpy gives"""
    c = case(name)
    e = exact_expected(c)
    failed = []
    if c["E"]:
        if not same_bits(np.asarray(out["colors"])[:, 3:], e["extras"], nan_payload=True):
            failed.append("extras")
        if not same_bits(out["d_extra"], e["d_extra"]):
            failed.append("d_extra")
    if c["deg"] == 0:
        if not same_bits(np.asarray(out["colors"])[:, :3], e["rgb"]):
            failed.append("rgb")
        if not same_bits(out["d_f_dc"], e["d_f_dc"]):
            failed.append("d_f_dc")
    if c["SC"] == 1:
        s = np.asarray(out["scales"])
        if not (same_bits(s[:, 0], s[:, 1], True) and same_bits(s[:, 0], s[:, 2], True)):
            failed.append("isotropic scales")
    return failed


# ---- the float32 model of the two kernels ------------------------------------------------------------------------------------------

# deliberate defects of model32 / stats_model: name -> (what is wrong, the case that shows it, the check that fails)
WRONG = {
    "tail_short": ("the tail quad stores one element too few", "cw3_p255_deg0", "bounded"),
    "tail_long": ("the tail quad stores one element too many", "cw3_p255_deg0", "past_end"),
    "row_advance": ("the row is not advanced when a quad crosses into the next row", "cw5_p204_deg2", "bounded"),
    "launch_P": ("the launch has P items", "cw8_p128_deg0of3", "bounded"),
    "launch_quads": ("the launch has ceil(P CW / 4) items", "cw3_p257_deg1", "bounded"),
    "clamp_gt": ("the clamp passes the gradient at raw > 0 only", "clamp0", "exact"),
    "dxyz_no_half": ("the d_xyz clamp decision is taken without the + 0.5", "cw4_p256_deg3", "consistency"),
    "frest_unwritten": ("d_f_rest beyond the active degree is not written", "cw4_p255_deg1of3", "bounded"),
    "sc1_one_column": ("the isotropic d_scaling is one column's product, not the sum of three", "cw3_p256_deg0of3", "bounded"),
    "normalize_below_eps": ("the projection term of d normalize is kept below the eps", "saturation_deg0", "bounded"),
    "sigmoid_no_1ms": ("1 - s dropped from d sigmoid", "cw4_p257_deg0", "bounded"),
    "sh_deg1": ("the sign of B_2 flipped", "onehot_deg1", "bounded"),
    "sh_deg2": ("B_6 with + xx", "onehot_deg2", "bounded"),
    "sh_deg3": ("B_12 with 3 zz for 2 zz", "onehot_deg3", "bounded"),
    "sh_grad": ("dB_11/dy with - yy for - 3 yy", "onehot_deg3", "bounded"),
    "dextra_CW": ("d_extra indexed with the row stride CW, not E", "cw5_p205_deg0", "exact"),
    "stats_reverse": ("the views are summed last to first", "stats", "stats"),
    "stats_radii0": ("a view with radii == 0 counts as seen", "stats", "stats"),
    "stats_rewrite": ("rows no view sees are written", "stats", "stats"),
}
GUARD = 64


def _basis32(deg, x, y, z, wrong):
    """sh_basis / sh_basis_grad of activations.hip in float32 numpy: B [P, 16], dB [P, 16, 3]"""
    f = F32
    P = x.shape[0]
    B, dB = np.zeros((P, 16), f), np.zeros((P, 16, 3), f)
    c1 = f(C1)
    c2, c3 = [f(v) for v in C2], [f(v) for v in C3]
    B[:, 0] = f(C0)
    if deg > 0:
        B[:, 1], B[:, 2], B[:, 3] = -c1 * y, (-c1 if wrong == "sh_deg1" else c1) * z, -c1 * x
        dB[:, 1, 1], dB[:, 2, 2], dB[:, 3, 0] = -c1, c1, -c1
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B[:, 4], B[:, 5] = c2[0] * xy, c2[1] * yz
        B[:, 6] = c2[2] * ((f(2) * zz + xx - yy) if wrong == "sh_deg2" else (f(2) * zz - xx - yy))
        B[:, 7], B[:, 8] = c2[3] * xz, c2[4] * (xx - yy)
        dB[:, 4, 0], dB[:, 4, 1] = c2[0] * y, c2[0] * x
        dB[:, 5, 1], dB[:, 5, 2] = c2[1] * z, c2[1] * y
        dB[:, 6, 0], dB[:, 6, 1], dB[:, 6, 2] = c2[2] * f(-2) * x, c2[2] * f(-2) * y, c2[2] * f(4) * z
        dB[:, 7, 0], dB[:, 7, 2] = c2[3] * z, c2[3] * x
        dB[:, 8, 0], dB[:, 8, 1] = c2[4] * f(2) * x, c2[4] * f(-2) * y
    if deg > 2:
        B[:, 9] = c3[0] * y * (f(3) * xx - yy)
        B[:, 10] = c3[1] * xy * z
        B[:, 11] = c3[2] * y * (f(4) * zz - xx - yy)
        B[:, 12] = c3[3] * z * ((f(3) if wrong == "sh_deg3" else f(2)) * zz - f(3) * xx - f(3) * yy)
        B[:, 13] = c3[4] * x * (f(4) * zz - xx - yy)
        B[:, 14] = c3[5] * z * (xx - yy)
        B[:, 15] = c3[6] * x * (xx - f(3) * yy)
        dB[:, 9, 0], dB[:, 9, 1] = c3[0] * f(6) * xy, c3[0] * (f(3) * xx - f(3) * yy)
        dB[:, 10, 0], dB[:, 10, 1], dB[:, 10, 2] = c3[1] * yz, c3[1] * xz, c3[1] * xy
        dB[:, 11, 0] = c3[2] * f(-2) * xy
        dB[:, 11, 1] = c3[2] * (f(4) * zz - xx - (f(1) if wrong == "sh_grad" else f(3)) * yy)
        dB[:, 11, 2] = c3[2] * f(8) * yz
        dB[:, 12, 0], dB[:, 12, 1] = c3[3] * f(-6) * xz, c3[3] * f(-6) * yz
        dB[:, 12, 2] = c3[3] * (f(6) * zz - f(3) * xx - f(3) * yy)
        dB[:, 13, 0], dB[:, 13, 1], dB[:, 13, 2] = c3[4] * (f(4) * zz - f(3) * xx - yy), c3[4] * f(-2) * xy, c3[4] * f(8) * xz
        dB[:, 14, 0], dB[:, 14, 1], dB[:, 14, 2] = c3[5] * f(2) * xz, c3[5] * f(-2) * yz, c3[5] * (xx - yy)
        dB[:, 15, 0], dB[:, 15, 1] = c3[6] * (f(3) * xx - f(3) * yy), c3[6] * f(-6) * xy
    return B, dB


def model32(c, wrong=None):
    """activate_fwd_kernel + activate_bwd_kernel as written, in float32 numpy: every output starts as NaN (an element no work item
    writes stays NaN), the colour table and dL/dcolors are walked quad by quad, work item t < P also owns Gaussian t.  Returns
    the outputs by name and `past_end`: was anything stored beyond an output's last element."""
    assert wrong is None or wrong in WRONG, wrong
    f = F32
    P, K, deg, SC, E = c["P"], c["K"], c["deg"], c["SC"], c["E"]
    CW, M = 3 + E, (deg + 1) ** 2
    total = P * CW
    quads = (total + 3) // 4
    items = P if wrong == "launch_P" else quads if wrong == "launch_quads" else max(quads, P)
    with np.errstate(all="ignore"):
        feats = np.concatenate([c["f_dc"], c["f_rest"]], axis=1).astype(f)           # [P, K, 3]
        if deg > 0:
            v = (c["xyz"] - c["campos"][None]).astype(f)
            vlen = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            x, y, z = v[:, 0] / vlen, v[:, 1] / vlen, v[:, 2] / vlen
            B, dB = _basis32(deg, x, y, z, wrong)
            acc = np.zeros((P, 3), f)
            for k in range(M):
                acc = acc + B[:, k, None] * feats[:, k, :]
            sh_sum, raw = acc, acc + f(0.5)
        else:
            B = np.zeros((P, 16), f)
            B[:, 0] = f(C0)
            raw = (f(C0) * feats[:, 0, :]).astype(f) + f(0.5)
        nan = lambda *s: np.full(s, np.nan, f)  # noqa: E731
        out = {"scales": nan(P, 3), "rotations": nan(P, 4), "opacities": nan(P, 1), "d_scaling": nan(P, SC), "d_rotation": nan(P, 4),
               "d_opacity": nan(P, 1), "d_f_dc": nan(P, 1, 3), "d_f_rest": nan(P, K - 1, 3), "d_xyz": nan(P, 3) if deg > 0 else None}
        colors, d_extra = nan(total + GUARD), nan(P * E + GUARD)
        gcol = c["G_colors"].astype(f).ravel()
        ext = None if not E else c["extra"].astype(f)
        past_end = False
        for t in range(items):
            if 4 * t >= total:
                continue
            row, col = divmod(4 * t, CW)
            vq = [f(0)] * 4
            frow, fcol = row, col
            for e in range(4):
                if 4 * t + e < total:
                    vq[e] = ext[frow, fcol - 3] if fcol >= 3 else max(raw[frow, fcol], f(0)) if raw[frow, fcol] == raw[frow, fcol] else f(0)
                fcol += 1
                if fcol == CW:
                    fcol = 0
                    if wrong != "row_advance":
                        frow += 1
            if 4 * t + 3 < total:
                colors[4 * t:4 * t + 4] = vq
            else:
                end = total + (1 if wrong == "tail_long" else -1 if wrong == "tail_short" else 0)
                for e in range(4):
                    if 4 * t + e < end:
                        colors[4 * t + e] = vq[e]
            for e in range(4):
                if 4 * t + e < total:
                    gq = gcol[4 * t + e]
                    if col >= 3:
                        idx = row * (CW if wrong == "dextra_CW" else E) + col - 3
                        if idx < d_extra.size:
                            d_extra[idx] = gq
                        else:
                            past_end = True
                    else:
                        passes = raw[row, col] > 0 if wrong == "clamp_gt" else raw[row, col] >= 0
                        gg = gq if passes else f(0)
                        out["d_f_dc"][row, 0, col] = B[row, 0] * gg
                        for k in range(1, K):
                            if k < M:
                                out["d_f_rest"][row, k - 1, col] = B[row, k] * gg
                            elif wrong != "frest_unwritten":
                                out["d_f_rest"][row, k - 1, col] = f(0)
                col += 1
                if col == CW:
                    col = 0
                    if wrong != "row_advance":
                        row += 1
        past_end = past_end or not np.isnan(colors[total:]).all() or not np.isnan(d_extra[P * E:]).all()
        n_g = min(items, P)
        sca = c["scaling"].astype(f)
        s = np.exp(sca)
        s3 = np.repeat(s, 3, axis=1) if SC == 1 else s
        q, gr = c["rotation"].astype(f), c["G_rotations"].astype(f)
        r = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
        n = np.maximum(r, f(EPS))
        u = q / n
        op = c["opacity"].astype(f)
        sig = f(1) / (f(1) + np.exp(-op))
        out["scales"][:n_g], out["rotations"][:n_g], out["opacities"][:n_g] = s3[:n_g], u[:n_g], sig[:n_g]
        gs = c["G_scales"].astype(f)
        if SC == 3:
            out["d_scaling"][:n_g] = (gs * s)[:n_g]
        else:
            out["d_scaling"][:n_g] = ((gs[:, :1] if wrong == "sc1_one_column" else (gs[:, :1] + gs[:, 1:2]) + gs[:, 2:3]) * s)[:n_g]
        ug = (((u[:, 0] * gr[:, 0] + u[:, 1] * gr[:, 1]) + u[:, 2] * gr[:, 2]) + u[:, 3] * gr[:, 3])[:, None]
        d_rot = (gr - u * ug) / n
        if wrong != "normalize_below_eps":
            d_rot = np.where(r < f(EPS), gr / f(EPS), d_rot)
        out["d_rotation"][:n_g] = d_rot[:n_g]
        go = c["G_opacities"].astype(f)
        out["d_opacity"][:n_g] = (go * sig if wrong == "sigmoid_no_1ms" else go * sig * (f(1) - sig))[:n_g]
        if deg > 0:
            dec = sh_sum if wrong == "dxyz_no_half" else raw
            gcc = np.where(dec >= 0, c["G_colors"][:, :3].astype(f), f(0))
            gx = np.zeros((P, 3), f)
            for k in range(1, M):
                w = (feats[:, k, 0] * gcc[:, 0] + feats[:, k, 1] * gcc[:, 1]) + feats[:, k, 2] * gcc[:, 2]
                gx = gx + dB[:, k, :] * w[:, None]
            dvec = np.stack([x, y, z], 1)
            dg = ((x * gx[:, 0] + y * gx[:, 1]) + z * gx[:, 2])[:, None]
            out["d_xyz"][:n_g] = ((gx - dvec * dg) / vlen[:, None])[:n_g]
    out["colors"] = colors[:total].reshape(P, CW)
    out["d_extra"] = d_extra[:P * E].reshape(P, E) if E else None
    out["past_end"] = past_end
    return out


# ---- named, seeded cases -----------------------------------------------------------------------------------------------------------

CAMPOS = np.array([0.25, -0.5, 1.0], F32)
NEAR_CAP = 0.05
F_DC_ZERO = F32(-1.7724538)          # fl(fl(C0 f) + 0.5) == 0.0 exactly; its float32 neighbours give -5.96e-8 and +2.98e-8
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


def item_count(P, CW):
    return max((P * CW + 3) // 4, P)


def _random_case(name, P, CW, deg, K, SC, seed, edge, near_rows=0):
    E = CW - 3
    g = np.random.default_rng(seed)
    nrm = lambda *s: g.standard_normal(s).astype(F32)  # noqa: E731
    c = {"name": name, "edge": edge, "P": P, "K": K, "deg": deg, "SC": SC, "E": E, "campos": CAMPOS.copy(),
         "xyz": (CAMPOS[None] + 3 * nrm(P, 3)).astype(F32), "f_dc": nrm(P, 1, 3), "f_rest": (0.5 * nrm(P, K - 1, 3)).astype(F32),
         "scaling": (nrm(P, SC) - 3).astype(F32), "rotation": nrm(P, 4), "opacity": (2 * nrm(P, 1)).astype(F32),
         "extra": g.random((P, E)).astype(F32) if E else None}
    if E:
        c["extra"][0, 0] = F32(-0.0)
    _gradients(c, g)
    if deg > 0 and near_rows:
        _plant_near_rows(c, near_rows)
    return c


def _gradients(c, g):
    P, E = c["P"], c["E"]
    nz = lambda a: np.where(np.abs(a) < 1e-3, F32(1e-3), a).astype(F32)  # noqa: E731
    c["G_scales"], c["G_rotations"] = nz(g.standard_normal((P, 3))), nz(g.standard_normal((P, 4)))
    c["G_opacities"], c["G_colors"] = nz(g.standard_normal((P, 1))), nz(g.standard_normal((P, 3 + E)))


def _raw64(c):
    """float64 raw = eval_sh + 0.5 [P, 3] of a case (numpy, from the monomial table)"""
    P, M = c["P"], (c["deg"] + 1) ** 2
    v = c["xyz"].astype(np.float64) - c["campos"].astype(np.float64)[None]
    d = v / np.sqrt((v * v).sum(1, keepdims=True)) if c["deg"] > 0 else np.zeros((P, 3))
    feats = np.concatenate([c["f_dc"], c["f_rest"]], axis=1).astype(np.float64)
    raw = np.full((P, 3), 0.5)
    for k in range(M):
        Bk = sum(coef * _mono((d[:, 0], d[:, 1], d[:, 2]), powers, np) for coef, powers in SH_TABLE[k])
        raw += Bk[:, None] * feats[:, k, :]
    return raw


def _plant_near_rows(c, rows):
    """the first `rows` rows, channel (row mod 3): f_dc moved so that the float64 raw lies a few float32 ulps of the terms from 0,
    on either side in turn (searched on the CPU: f_dc is float32, so raw lands where it lands; the side is then read back)"""
    for _ in range(3):
        raw = _raw64(c)
        for i in range(rows):
            ch = i % 3
            want = (1 if i % 2 else -1) * 3e-8
            c["f_dc"][i, 0, ch] = F32(c["f_dc"][i, 0, ch] - (raw[i, ch] - want) / C0)
    raw = _raw64(c)
    got = np.array([raw[i, i % 3] for i in range(rows)])
    assert (np.abs(got) < 4e-7).all() and (got > 0).any() and (got < 0).any(), got


def _onehot_case(name, deg, edge):
    """row (k, direction): coefficient k alone is nonzero, the direction one of the 6 axes and 8 cube diagonals, at an exact distance of 2
    along an axis; amplitudes small enough that every channel passes the clamp (|B_k| < 2)"""
    dirs = np.array(AXES + DIAGONALS, np.float64)
    P = 16 * len(dirs)
    g = np.random.default_rng(77)
    c = {"name": name, "edge": edge, "P": P, "K": 16, "deg": deg, "SC": 3, "E": 0, "campos": CAMPOS.copy(), "extra": None}
    c["xyz"] = (CAMPOS[None].astype(np.float64) + 2.0 * np.tile(dirs, (16, 1))).astype(F32)
    feats = np.zeros((P, 16, 3), F32)
    for k in range(16):
        feats[k * len(dirs):(k + 1) * len(dirs), k, :] = np.array([0.25, -0.125, 0.0625], F32)
    c["f_dc"], c["f_rest"] = feats[:, :1].copy(), feats[:, 1:].copy()
    c["scaling"] = (g.standard_normal((P, 3)) - 3).astype(F32)
    c["rotation"] = g.standard_normal((P, 4)).astype(F32)
    c["opacity"] = g.standard_normal((P, 1)).astype(F32)
    _gradients(c, g)
    return c


def _clamp0_case(name, edge):
    """degree 0: every channel of 9 rows at F_DC_ZERO or one of its float32 neighbours"""
    below, above = np.nextafter(F_DC_ZERO, F32(-np.inf)), np.nextafter(F_DC_ZERO, F32(np.inf))
    c = _random_case(name, 9, 4, 0, 1, 3, 31, edge)
    vals = np.array([below, F_DC_ZERO, above], F32)
    for i in range(9):
        c["f_dc"][i, 0, :] = vals[[(i + ch * (i // 3)) % 3 for ch in range(3)]]
    return c


def _saturation_case(name, deg, K, SC, edge):
    """logits of +-20, +-88, +-90, +-inf; log-scales at 88.7 (the last finite expf), 88.73, 89 and 100 (infinite), -87 (the last normal one),
    -104 and -110 (zero); quaternions scaled by 1e-6 .. 1e6, a zero one, norms of 0.99e-12 and 1.01e-12 and (3e-14, 4e-14, 0, 0)"""
    logits = [20, -20, 88, -88, 90, -90, np.inf, -np.inf, 0, 3]
    lscales = [88.7, 88.73, 89, 100, -87, -104, -110, 0, -3, 2]
    P = 40
    c = _random_case(name, P, 4, deg, K, SC, 41, edge)
    c["opacity"][:, 0] = np.array([logits[i % len(logits)] for i in range(P)], F32)
    for i in range(P):
        c["scaling"][i, :] = c["scaling"][i, :] * F32(0.001) + F32(lscales[(i // 2) % len(lscales)])     # +- 0.006 at the most
    unit = c["rotation"] / np.sqrt((c["rotation"].astype(np.float64) ** 2).sum(1, keepdims=True))
    for i, s in enumerate([1e-6, 1e-3, 1.0, 1e3, 1e6]):
        c["rotation"][i] = (unit[i] * s).astype(F32)
        c["rotation"][5 + i] = (unit[i] * s).astype(F32)            # the same direction at every scale: rows 5.. repeat rows 0..
    c["rotation"][10] = 0
    c["rotation"][11] = (unit[11] * 0.99e-12).astype(F32)
    c["rotation"][12] = (unit[12] * 1.01e-12).astype(F32)
    c["rotation"][13] = np.array([3e-14, 4e-14, 0, 0], F32)
    c["G_rotations"][13] = np.array([1, 2, 3, 4], F32)
    c["rotation"][14] = np.array([0, 0, 0, 5e-13], F32)
    return c


def _small(name, P, CW, deg, K, SC, seed):
    return lambda: _random_case(name, P, CW, deg, K, SC, seed, f"P = {P}: {item_count(P, CW)} item(s), tail of {P * CW % 4}")


def _quad(name, P, CW, deg, K, SC, seed):
    near = int(NEAR_CAP * P) - 2 if deg > 0 and int(NEAR_CAP * P) >= 4 else 0       # two rows of the cap left to chance
    return lambda: _random_case(name, P, CW, deg, K, SC, seed,
                                f"{item_count(P, CW)} items for {P} Gaussians and {(P * CW + 3) // 4} quads, tail of {P * CW % 4}", near)


# CW = 35: 35 P / 4 moves in steps of 8.75, no P gives 255 .. 257 items: 29 gives 254, 30 gives 263 (the workgroup boundary lies between)
CASES = {
    "cw3_p255_deg0": _quad("cw3_p255_deg0", 255, 3, 0, 1, 3, 1), "cw3_p256_deg0of3": _quad("cw3_p256_deg0of3", 256, 3, 0, 16, 1, 2),
    "cw3_p257_deg1": _quad("cw3_p257_deg1", 257, 3, 1, 4, 3, 3),
    "cw4_p255_deg1of3": _quad("cw4_p255_deg1of3", 255, 4, 1, 16, 1, 4), "cw4_p256_deg3": _quad("cw4_p256_deg3", 256, 4, 3, 16, 3, 5),
    "cw4_p257_deg0": _quad("cw4_p257_deg0", 257, 4, 0, 1, 1, 6),
    "cw5_p204_deg2": _quad("cw5_p204_deg2", 204, 5, 2, 9, 3, 7), "cw5_p205_deg0": _quad("cw5_p205_deg0", 205, 5, 0, 1, 3, 8),
    "cw8_p128_deg0of3": _quad("cw8_p128_deg0of3", 128, 8, 0, 16, 3, 9), "cw8_p128_deg2of3": _quad("cw8_p128_deg2of3", 128, 8, 2, 16, 1, 10),
    "cw35_p29_deg1": _quad("cw35_p29_deg1", 29, 35, 1, 4, 3, 11), "cw35_p30_deg0": _quad("cw35_p30_deg0", 30, 35, 0, 1, 3, 12),
    "p1_cw3_deg3": _small("p1_cw3_deg3", 1, 3, 3, 16, 3, 13), "p2_cw5_deg2": _small("p2_cw5_deg2", 2, 5, 2, 9, 1, 14),
    "p2_cw3_deg1": _small("p2_cw3_deg1", 2, 3, 1, 4, 3, 15), "p3_cw4_deg0": _small("p3_cw4_deg0", 3, 4, 0, 1, 3, 16),
    "p5_cw35_deg0": _small("p5_cw35_deg0", 5, 35, 0, 4, 1, 17), "p5_cw8_deg3": _small("p5_cw8_deg3", 5, 8, 3, 16, 3, 18),
    "onehot_deg0": lambda: _onehot_case("onehot_deg0", 0, "K = 16 at degree 0: fifteen rows of zeros per Gaussian in d_f_rest"),
    "onehot_deg1": lambda: _onehot_case("onehot_deg1", 1, "every basis function of degree 1 alone, K = 16"),
    "onehot_deg2": lambda: _onehot_case("onehot_deg2", 2, "every basis function up to degree 2 alone, K = 16"),
    "onehot_deg3": lambda: _onehot_case("onehot_deg3", 3, "every basis function and derivative alone, on the axes and the cube diagonals"),
    "clamp0": lambda: _clamp0_case("clamp0", "degree 0 at raw == 0 exactly and one ulp of f_dc to either side"),
    "saturation_deg0": lambda: _saturation_case("saturation_deg0", 0, 1, 3, "saturated logits and log-scales, quaternions at the eps"),
    "saturation_deg2": lambda: _saturation_case("saturation_deg2", 2, 9, 1, "the same at degree 2 with an isotropic scale"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case: float32 arrays, shared, never modified.  Asserts the near-row cap on the reference alone."""
    c = CASES[name]()
    for k in INPUTS:
        if c[k] is not None:
            c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference_of(name):
    ref = reference(case(name))
    assert near_rows(name, ref) <= NEAR_CAP * case(name)["P"], (name, near_rows(name, ref))
    return ref


def near_rows(name, ref=None):
    """rows of a case with a colour channel the float64 reference cannot decide the clamp for"""
    ref = reference_of(name) if ref is None else ref
    return int(ref["near"].any(1).sum())


def raw_path_rows():
    """rows of the saturation, clamp and one degree-0 quad case that keep the rasterizer finite: the logits, the clamp triple, the
    scaled quaternions and the sub-eps quaternions, all with ordinary log-scales (raw inputs by name, float32)"""
    sat, cl = case("saturation_deg0"), case("clamp0")
    n = sat["P"] + cl["P"]
    out = {"scaling": np.full((n, 3), -3.0, F32), "rotation": np.concatenate([sat["rotation"], cl["rotation"]]),
           "opacity": np.concatenate([sat["opacity"], cl["opacity"]]), "f_dc": np.concatenate([sat["f_dc"], cl["f_dc"]]),
           "extra": np.concatenate([sat["extra"], cl["extra"]])}
    out["scaling"] += np.linspace(-0.5, 0.5, n, dtype=F32)[:, None]
    return out


# ---- densification statistics -------------------------------------------------------------------------------------------------------

TRIPLES = ((3, 4), (5, 12), (8, 15), (7, 24), (20, 21), (0, 7), (9, 0), (6, 8))


@functools.lru_cache(maxsize=None)
def stats_case(P, V, seed=0):
    """view-space gradients whose gx^2 + gy^2 and its root are exact in float32 (Pythagorean integers times a power of two between
    2^-3 and 2^26: the running sum rounds, in view order), a NaN in the unused third column; radii with zeros and negatives; a
    quarter of the rows seen by no view, their state seeded with NaN and -0"""
    g = np.random.default_rng(1000 * P + V + seed)
    grads, radii = [], []
    unseen = (np.arange(P) % 4 == 1)
    for v in range(V):
        t = np.array(TRIPLES)[g.integers(0, len(TRIPLES), P)]
        scale = np.exp2(g.integers(-3, 27, P)).astype(np.float64)
        sign = g.choice([-1.0, 1.0], (P, 2))
        gr = np.full((P, 3), np.nan, F32)
        gr[:, :2] = (t * sign * scale[:, None]).astype(F32)
        r = g.integers(-2, 40, P).astype(np.int32)
        r[unseen] = np.where(r[unseen] > 0, np.int32(0) if v % 2 else np.int32(-3), r[unseen])
        grads.append(gr)
        radii.append(r)
    seen_any = np.any([r > 0 for r in radii], axis=0)
    accum = g.integers(0, 50, P).astype(F32)
    denom = g.integers(0, 9, P).astype(F32)
    maxr = g.integers(0, 30, P).astype(F32)
    seed_vals = np.where(np.arange(P) % 8 < 4, F32(np.nan), F32(-0.0)).astype(F32)
    for a in (accum, denom, maxr):
        a[~seen_any] = seed_vals[~seen_any]
    return {"P": P, "V": V, "grads": grads, "radii": radii, "accum": accum, "denom": denom, "max_radii": maxr, "seen": seen_any}


def stats_model(s, only_max=False, wrong=None):
    """densification_stats_kernel in float32 numpy, sequentially in view order -> (accum, denom, max_radii); the first two are the
    inputs unchanged when only_max"""
    f = F32
    P = s["P"]
    accum, denom, maxr = s["accum"].copy(), s["denom"].copy(), s["max_radii"].copy()
    order = range(s["V"] - 1, -1, -1) if wrong == "stats_reverse" else range(s["V"])
    for i in range(P):
        a = n = m = f(0)
        seen = False
        for v in order:
            r = s["radii"][v][i]
            if (r < 0) if wrong == "stats_radii0" else (r <= 0):
                continue
            if not seen:
                seen, m = True, maxr[i]
                if not only_max:
                    a, n = accum[i], denom[i]
            if not only_max:
                gx, gy = s["grads"][v][i, 0], s["grads"][v][i, 1]
                a = f(a + np.sqrt(f(f(gx * gx) + f(gy * gy))))
                n = f(n + f(1))
            m = max(m, f(r))
        if seen or wrong == "stats_rewrite":
            maxr[i] = m
            if not only_max:
                accum[i], denom[i] = a, n
    return accum, denom, maxr


def check_stats(run, P, V):
    """`run(grads, radii, accum, denom, max_radii)` updates copies in place (accum = denom = None: max_radii only) and is held, bit for
    bit, to the sequential model; failures by name"""
    s = stats_case(P, V)
    failed = []
    for only_max in (False, True):
        accum, denom, maxr = s["accum"].copy(), s["denom"].copy(), s["max_radii"].copy()
        got = run(s["grads"], s["radii"], None if only_max else accum, None if only_max else denom, maxr)
        accum, denom, maxr = got if got is not None else (accum, denom, maxr)
        ea, ed, em = stats_model(s, only_max)
        for k, a, b in (("accum", accum, ea), ("denom", denom, ed), ("max_radii", maxr, em)):
            if only_max and k != "max_radii":
                continue
            if not same_bits(a, b):
                failed.append(f"{k}{' (max only)' if only_max else ''}")
            if not same_bits(np.asarray(a)[~s["seen"]], s[k][~s["seen"]]):
                failed.append(f"{k} of unseen rows{' (max only)' if only_max else ''}")
    return failed
