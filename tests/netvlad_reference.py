"""Oracle, restatement, bars, cases and wrong models of the NetVLAD head tests (tests/test_host_netvlad_head.py,
tests/test_gpu_netvlad_head.py): splatloc_amd/netvlad.py over csrc/netvlad_head.hip.

hloc's NetVLAD layer is not in the reference tree, so include/splatraster.h (splatraster_netvlad_*) and INTEGRATION.md §25 are the
contract.  This file holds

* the float64 ORACLE of the contract, stage by stage (`assign64`, `aggregate64`, `project64`), each from float32 stage inputs, so
  that a stage can be held to the oracle on the previous stage's own output (the device's, or the restatement's);
* the float32 RESTATEMENT from torch CPU operators in hloc's literal form (`restatement`): F.normalize, a 1x1 convolution,
  F.softmax, (a.unsqueeze(1) * (x.unsqueeze(2) - c)).sum(-1), F.normalize twice, F.linear, F.normalize;
* the BARS.  `aggregate` raw and `project` raw are elementwise and derived, gamma(n) * sum|terms| with gamma(n) = n u / (1 - n u),
  u = 2^-24 (+ 2^-126 where the terms are not all zero: a result below the normal range may be flushed):
    aggregate raw   sum|terms| = sum_n |a xh| + |c| sum_n a, n = N + 3: xh's own rounding, at most N roundings on the way through
                    a sum of N products in any order, the centre product, the subtraction
    project raw     sum|terms| = sum_i |w x| + |bias|, n = I + 2
  A normalisation y = v / max(||v||, 1e-12) of an input v known to e elementwise (`normalize64`): the denominator is 1-Lipschitz
  in v, so it moves by at most ||e||_2, to den_lo = max(den - ||e||_2, 1e-12) at the least, and
    bar = e / den_lo + |v| ||e||_2 / (den den_lo) + gamma(L + 6) (|v| + e) / den_lo
  with L the length of the normalised axis: L + 1 roundings in the sum of squares, the root and the division counted twice each.
  `assign` depends on the device's expf, whose error cannot be derived here: the project's existing rule (SuperPoint head, loss
  stage), per case four times the restatement's own maximum error against the oracle: absolute for assign, relative for inv_norm
  (an all-zero location has inv_norm = 1e12 beside values near 1).  Where the restatement is exact the device must be;
* the EXACT family (`exact_case`): columns with a single +-2^j entry (inv_norm and xh exact), score_w = 0 (a = 1 / K exactly for a
  power of two K), dyadic centres, weights and biases small enough that every sum is exact in float32 under any order: oracle,
  restatement and device agree bit for bit on assign, inv_norm, the raw V and the raw projection;
* WRONG models: float64 variants of the oracle (one in float32, where its defect lives) with one deliberate defect each, and the
  case and output on which each must exceed the bar;
* named, seeded cases (`CASES`), each with the edge it exists for.  The tile constants the shapes sit at are those of
  splatraster_netvlad_tiles; both test files assert that the library reports the same.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-12
INTRANORM, L2NORM = 1, 2

# splatraster_netvlad_tiles: locations per step, d rows per workgroup, I slice, o rows and b columns of a projection tile
T, D_TILE, I_SLICE, O_TILE, B_TILE = 64, 32, 2048, 128, 32
TILES = {"n_step": T, "d_tile": D_TILE, "i_slice": I_SLICE, "o_tile": O_TILE, "b_tile": B_TILE}


def gamma(n):
    """n roundings of relative size 2^-24 each, compounded (Higham's gamma_n)"""
    return n * U / (1.0 - n * U)


# ---- the float64 oracle, stage by stage ----------------------------------------------------------------------------------------------

def assign64(x, score_w, score_b, wrong=None):
    """(assign [B,K,N], inv_norm [B,N]) in float64 of float32 inputs"""
    x, w = x.double(), score_w.double()
    nrm = x.pow(2).sum(2 if wrong == "norm_over_N" else 1, keepdim=True).sqrt()
    inv = 1.0 / (nrm if wrong == "no_eps" else nrm.clamp_min(EPS))
    xh = x * inv
    s = torch.einsum("kd,bdn->bkn", w, xh)
    if score_b is not None and wrong != "bias_dropped":
        s = s + score_b.double()[None, :, None]
    if wrong == "no_max":                                   # the defect lives in float32: expf of the unshifted logits
        e = torch.exp(s.float())
        a = (e / e.sum(1, keepdim=True)).double()
    else:
        a = F.softmax(s, 2 if wrong == "softmax_over_N" else 1)
    inv_out = inv[:, :1, 0].expand(x.shape[0], x.shape[2]) if wrong == "norm_over_N" else inv[:, 0]
    return a, inv_out.contiguous()


def normalize64(v, e, dim, wrong=None):
    """y = v / max(||v||, eps) along `dim` and its bar for an input known to `e` elementwise (module docstring)"""
    L = v.shape[dim]
    nrm = v.pow(2).sum(dim, keepdim=True).sqrt()
    den = nrm if wrong == "no_eps" else nrm.clamp_min(EPS)
    en = e.pow(2).sum(dim, keepdim=True).sqrt()
    den_lo = (den - en).clamp_min(EPS)
    y = v / den
    bar = e / den_lo + v.abs() * en / (den * den_lo) + gamma(L + 6) * (v.abs() + e) / den_lo
    return y, bar + TINY * (bar > 0)


def aggregate64(x, a, inv, centers, flags, wrong=None):
    """{"v" [B, D K], "bar"} of float32 stage inputs: features, assign, inv_norm, centers"""
    x, a, inv, c = x.double(), a.double(), inv.double(), centers.double()
    B, D, N = x.shape
    K = a.shape[1]
    xh = x * inv[:, None, :]
    n_used = (N - 1) // T * T if wrong == "last_step_dropped" else N
    S = torch.einsum("bkn,bdn->bdk", a[:, :, :n_used], xh[:, :, :n_used])
    sa = a[:, :, :n_used].sum(2)                                                     # [B,K]
    V = S - c[None] * (float(N) if wrong == "centre_times_N" else sa[:, None, :])
    if wrong == "last_d_block_dropped":
        V[:, (D - 1) // D_TILE * D_TILE:] = 0.0
    terms = torch.einsum("bkn,bdn->bdk", a.abs(), xh.abs()) + c.abs()[None] * a.abs().sum(2)[:, None, :]
    bar = gamma(N + 3) * terms + TINY * (terms > 0)
    if flags & INTRANORM and wrong != "intranorm_skipped":
        V, bar = normalize64(V, bar, 1)
    V = (V.transpose(1, 2) if wrong == "flatten_kD" else V).reshape(B, D * K)
    bar = (bar.transpose(1, 2) if wrong == "flatten_kD" else bar).reshape(B, D * K)
    if flags & L2NORM:
        V, bar = normalize64(V, bar, 1)
    return {"v": V, "bar": bar}


def project64(x, weight, bias, flags, wrong=None):
    """{"y" [B,O], "bar"} of float32 stage inputs"""
    x, w = x.double(), weight.double()
    O, I = w.shape
    if wrong == "row_0":
        x = x[:1].expand_as(x)
    if wrong == "weight_transposed":
        w = w.reshape(I, O).t()
    i_used = (I - 1) // I_SLICE * I_SLICE if wrong == "last_slice_dropped" else I
    y = x[:, :i_used] @ w[:, :i_used].t()
    terms = x.abs() @ weight.double().abs().t()
    if bias is not None:
        terms = terms + bias.double().abs()[None]
        if wrong != "bias_after_norm":
            y = y + bias.double()[None]
    bar = gamma(I + 2) * terms + TINY * (terms > 0)
    if flags & L2NORM:
        y, bar = normalize64(y, bar, 1)
    if bias is not None and wrong == "bias_after_norm":
        y = y + bias.double()[None]
    return {"y": y, "bar": bar}


# ---- the float32 restatement in hloc's literal form ---------------------------------------------------------------------------------

def restatement(c):
    """The head of case `c` from torch CPU float32 operators, in the shape of a staged device run: assign, inv_norm, raw (the
    residual matrix, flattened), v (normalised), and with a whitening y_raw and y.  A project-only case gives y_raw and y of its x."""
    out = {}
    if "features" in c:
        x = c["features"]
        B, D, N = x.shape
        K = c["score_w"].shape[0]
        out["inv_norm"] = 1.0 / x.norm(dim=1).clamp_min(EPS)
        xh = F.normalize(x, p=2, dim=1)
        s = F.conv1d(xh, c["score_w"][:, :, None], c["score_b"])
        a = F.softmax(s, dim=1)
        out["assign"] = a
        raw = torch.stack([(a[b].unsqueeze(0) * (xh[b].unsqueeze(1) - c["centers"].unsqueeze(-1))).sum(-1) for b in range(B)])
        out["raw"] = raw.reshape(B, D * K)
        v = F.normalize(raw, p=2, dim=1) if c["intranorm"] else raw
        v = F.normalize(v.reshape(B, D * K), p=2, dim=1)
        out["v"] = v
    else:
        v = c["x"]
    if c.get("whiten_w") is not None:
        out["y_raw"] = F.linear(v, c["whiten_w"], c["whiten_b"])
        out["y"] = F.normalize(out["y_raw"], p=2, dim=1)
    return out


def flags_of(c):
    return (INTRANORM if c["intranorm"] else 0) | L2NORM


def oracle_chain(c, wrong=None):
    """the whole head in float64 from the case's inputs alone, every stage on the float32 rounding of the one before"""
    out = {}
    if "features" in c:
        a, inv = assign64(c["features"], c["score_w"], c["score_b"], wrong)
        out["assign"], out["inv_norm"] = a, inv
        a32, inv32 = a.float(), inv.float()
        out["raw"] = aggregate64(c["features"], a32, inv32, c["centers"], 0, wrong)["v"]
        r = aggregate64(c["features"], a32, inv32, c["centers"], flags_of(c), wrong)
        out["v"], out["v_bar"] = r["v"], r["bar"]
        x = r["v"].float()
    else:
        x = c["x"]
    if c.get("whiten_w") is not None:
        out["y_raw"] = project64(x, c["whiten_w"], c["whiten_b"], 0, wrong)["y"]
        r = project64(x, c["whiten_w"], c["whiten_b"], L2NORM, wrong)
        out["y"], out["y_bar"] = r["y"], r["bar"]
    return out


# ---- ratios ----------------------------------------------------------------------------------------------------------------------

def worst(got, ref, bar):
    """largest |got - ref| / bar.  Never NaN: an error above a zero bar, a NaN or an infinity counts as infinite."""
    got, ref, bar = (torch.as_tensor(t).double() for t in (got, ref, bar))
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    ok = err <= bar
    ratio = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)), torch.zeros_like(bar))
    ratio = torch.where(ok | (torch.isfinite(ratio) & (ratio > 1.0)), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def _err_abs(got, ref):
    e = (torch.as_tensor(got).double() - ref).abs()
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def _err_rel(got, ref):
    e = (torch.as_tensor(got).double() - ref).abs() / ref.abs()
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def _four_times(got, ref):
    """the 4x rule as a ratio: device error over four times the restatement's; an exact restatement asks for an exact device"""
    if ref == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return got / (4.0 * ref)


@functools.lru_cache(maxsize=None)
def assign_reference(name):
    """(oracle assign, oracle inv_norm, restatement's max abs error of assign, its max relative error of inv_norm) of a case"""
    c = case(name)
    a, inv = assign64(c["features"], c["score_w"], c["score_b"])
    r = restatement(c)
    return a, inv, _err_abs(r["assign"], a), _err_rel(r["inv_norm"], inv)


def ratios(name, out):
    """error / bar of every output in `out` (float32 CPU tensors by the names of `restatement`) on case `name`, each stage held to
    the oracle on `out`'s own output of the stage before"""
    c = case(name)
    r = {}
    if "assign" in out:
        a, inv, ea, ei = assign_reference(name)
        r["assign"] = _four_times(_err_abs(out["assign"], a), ea)
        r["inv_norm"] = _four_times(_err_rel(out["inv_norm"], inv), ei)
    for key, flags in (("raw", 0), ("v", None)):
        if key in out:
            ref = aggregate64(c["features"], out["assign"], out["inv_norm"], c["centers"], flags_of(c) if flags is None else flags)
            r[key] = worst(out[key], ref["v"], ref["bar"])
    for key, flags in (("y_raw", 0), ("y", L2NORM)):
        if key in out:
            ref = project64(out["v"] if "features" in c else c["x"], c["whiten_w"], c["whiten_b"], flags)
            r[key] = worst(out[key], ref["y"], ref["bar"])
    return r


def within(r):
    return all(v <= 1.0 for v in r.values())


def same_bits(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32).contiguous(), torch.as_tensor(b, dtype=torch.float32).contiguous()
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# ---- wrong models --------------------------------------------------------------------------------------------------------------------

# name -> (what is wrong, the case that shows it, the output whose bar it must exceed)
WRONG = {
    "no_eps": ("no eps in the normalisation", "zero_locations", "assign"),
    "norm_over_N": ("normalisation over N instead of D", "n65_d33_k1", "inv_norm"),
    "softmax_over_N": ("softmax over N instead of K", "n63_d31_k63", "assign"),
    "no_max": ("no max subtraction (float32)", "saturated", "assign"),
    "bias_dropped": ("dropped score bias", "n1_d3_k2", "assign"),
    "centre_times_N": ("centre term times N instead of sum a", "n64_d32_k64", "raw"),
    "flatten_kD": ("flatten order k * D + d", "n63_d31_k63", "v"),
    "intranorm_skipped": ("intranorm skipped", "n64_d32_k64", "v"),
    "last_step_dropped": ("last step of locations dropped", "n129_d1_k2", "raw"),
    "last_d_block_dropped": ("last d block dropped", "n65_d33_k1", "raw"),
    "bias_after_norm": ("bias added after the normalisation", "n1_d3_k2", "y"),
    "weight_transposed": ("weight read transposed", "i3_otile_m1", "y_raw"),
    "last_slice_dropped": ("last I slice dropped", "i2049_o3", "y_raw"),
    "row_0": ("row b reading row 0", "i2049_o3", "y_raw"),
}


def wrong_output(name):
    """(ratio of the wrong model's output against the bar, on the stage inputs of the oracle chain) for WRONG[name]"""
    _, cname, key = WRONG[name]
    c = case(cname)
    good = oracle_chain(c)
    if key in ("assign", "inv_norm"):
        a, inv = assign64(c["features"], c["score_w"], c["score_b"], name)
        out = {"assign": a, "inv_norm": inv}
        return ratios(cname, out)[key]
    out = {k: good[k].float() for k in ("assign", "inv_norm", "v") if k in good}
    if key in ("raw", "v"):
        flags = 0 if key == "raw" else flags_of(c)
        out[key] = aggregate64(c["features"], out["assign"], out["inv_norm"], c["centers"], flags, name)["v"]
    else:
        x = out["v"] if "features" in c else c["x"]
        out[key] = project64(x, c["whiten_w"], c["whiten_b"], 0 if key == "y_raw" else L2NORM, name)["y"]
    return ratios(cname, out)[key]


# ---- named, seeded cases -----------------------------------------------------------------------------------------------------------

def _head_case(name, edge, B, D, K, N, O, seed, score_bias=True, whiten_bias=True, intranorm=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = {"name": name, "edge": edge, "features": rn(B, D, N) * (0.5 + torch.rand(B, 1, N, generator=g)),
         "score_w": rn(K, D) * 2.0, "score_b": rn(K) * 0.5 if score_bias else None, "centers": rn(D, K) / max(D, 1) ** 0.5,
         "intranorm": intranorm, "whiten_w": None, "whiten_b": None}
    if O:
        c["whiten_w"] = rn(O, D * K) / (D * K) ** 0.5
        c["whiten_b"] = rn(O) * 0.1 if whiten_bias else None
    return c


def _project_case(name, edge, B, O, I, seed, bias=True, unaligned=False):
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(B, I, generator=g), dim=1)
    return {"name": name, "edge": edge, "x": x, "whiten_w": torch.randn(O, I, generator=g) / I ** 0.5,
            "whiten_b": torch.randn(O, generator=g) * 0.1 if bias else None, "unaligned": unaligned}


def _zero_locations(name, edge):
    c = _head_case(name, edge, 2, 8, 4, T + 3, 5, 101)
    c["features"][0, :, 0] = 0.0
    c["features"][0, :, T - 1:T + 1] = 0.0           # across the step edge
    c["features"][1, :, -1] = 0.0
    c["zero"] = [(0, 0), (0, T - 1), (0, T), (1, T + 2)]
    return c


def _zero_image(name, edge):
    c = _head_case(name, edge, 3, 5, 3, 70, 4, 102)
    c["features"][1] = 0.0
    return c


def _saturated(name, edge):
    """one-hot columns, so s[k, n] = score_w[k, d(n)] exactly: logits of +-80 (a one-hot assignment), a block with every logit
    near -95 (expf of the unshifted logit is subnormal) and a block near +92 (it overflows)"""
    D, K, N = 12, 4, 96
    g = torch.Generator().manual_seed(103)
    w = torch.full((K, D), -80.0)
    for d in range(4):
        w[d % K, d] = 80.0
    w[:, 4:8] = -95.0 + torch.randn(K, 4, generator=g)
    w[:, 8:12] = 92.0 + torch.randn(K, 4, generator=g)
    x = torch.zeros(1, D, N)
    for n in range(N):
        x[0, n % D, n] = float(2 ** (n % 5 - 2)) * (1 if n % 3 else -1) if n % D >= 4 else 1.5 + 0.125 * (n % 7)
    return {"name": name, "edge": edge, "features": x, "score_w": w, "score_b": None,
            "centers": torch.randn(D, K, generator=g) * 0.3, "intranorm": True,
            "whiten_w": torch.randn(6, D * K, generator=g) / (D * K) ** 0.5, "whiten_b": None}


def _retrieval(name, edge):
    """rows 0..39 the database, rows 40..45 the queries: database rows 3 q, 3 q + 1, 3 q + 2 are query q's map under one noise pattern of growing size,
    the other 22 rows are unrelated maps; small centres and no whitening bias"""
    B_DB, Q, D, K, N, O = 40, 6, 16, 8, 70, 32
    c = _head_case(name, edge, B_DB + Q, D, K, N, O, 104)
    g = torch.Generator().manual_seed(105)
    for q in range(Q):
        noise = torch.randn(D, N, generator=g)
        for j, sigma in enumerate((0.1, 0.3, 0.5)):
            c["features"][3 * q + j] = c["features"][B_DB + q] + sigma * noise
    c["centers"] = c["centers"] * 0.05         # residuals that follow the map, not the centres: descriptors that tell maps apart
    c["whiten_b"] = None
    c["n_db"], c["topk"] = B_DB, 3
    return c


def exact_case(name, edge, B, D, K, N, O, seed, bias):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)  # noqa: E731
    x = torch.zeros(B, D, N)
    ch = ri(0, D - 1, B, N)
    val = torch.exp2(ri(-8, 8, B, N).float()) * (2.0 * ri(0, 1, B, N).float() - 1.0)
    x.scatter_(1, ch[:, None, :], val[:, None, :])
    c = {"name": name, "edge": edge, "features": x, "score_w": torch.zeros(K, D), "score_b": torch.full((K,), 0.75) if bias else None,
         "centers": ri(-32, 32, D, K).float() / 8.0, "intranorm": True, "exact": True,
         "whiten_w": ri(-8, 8, O, D * K).float() / 4.0, "whiten_b": ri(-16, 16, O).float() / 8.0 if bias else None}
    return c


def exact_project_case(name, edge, B, O, I, seed, unaligned=False):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    return {"name": name, "edge": edge, "x": ri(-16, 16, B, I) / 8.0, "whiten_w": ri(-8, 8, O, I) / 4.0, "whiten_b": ri(-16, 16, O) / 8.0,
            "exact": True, "unaligned": unaligned}


CASES = {
    # N in {1, T-1, T, T+1, 2T+1}, D in {1, 3, d_tile-1, d_tile, d_tile+1}, K in {1, 2, 63, 64}, O in {1, o_tile-1, o_tile, o_tile+1},
    # B in {1, 2, b_tile, b_tile+1}
    "n1_d3_k2": lambda n: _head_case(n, "N = 1, D = 3, K = 2, O = 1, B = 1; both biases", 1, 3, 2, 1, 1, 1),
    "n63_d31_k63": lambda n: _head_case(n, "N = T - 1, D = d_tile - 1, K = 63, O = o_tile - 1, B = 2", 2, D_TILE - 1, 63, T - 1, O_TILE - 1, 2),
    "n64_d32_k64": lambda n: _head_case(n, "N = T, D = d_tile, K = 64, O = o_tile; no score bias", 1, D_TILE, 64, T, O_TILE, 3, score_bias=False),
    "n65_d33_k1": lambda n: _head_case(n, "N = T + 1, D = d_tile + 1, K = 1, O = o_tile + 1; no intranorm, no whitening bias", 2, D_TILE + 1, 1,
                                       T + 1, O_TILE + 1, 4, whiten_bias=False, intranorm=False),
    "n129_d1_k2": lambda n: _head_case(n, "N = 2 T + 1, D = 1, B = b_tile + 1", B_TILE + 1, 1, 2, 2 * T + 1, 2, 5),
    "b32_d3_k2": lambda n: _head_case(n, "B = b_tile", B_TILE, 3, 2, 5, 3, 6),
    "no_whitening": lambda n: _head_case(n, "a head without whitening: the descriptor is v", 2, 6, 4, 20, 0, 7),
    "layer": lambda n: _head_case(n, "the layer's own D = 512, K = 64, N = 1200 with O = 128", 2, 512, 64, 1200, 128, 8),
    "zero_locations": lambda n: _zero_locations(n, "all-zero locations, at a step edge too: a = softmax(score_b)"),
    "zero_image": lambda n: _zero_image(n, "an all-zero image between two others"),
    "saturated": lambda n: _saturated(n, "|s| near 80: one-hot assignment; logits near -95 and near +92"),
    "retrieval": lambda n: _retrieval(n, "descriptors whose top-k similarities are apart by 64 bars"),
    # I in {1, 3, slice-1, slice, slice+1, 2 slice+4}
    "i1_o1": lambda n: _project_case(n, "I = 1, O = 1, B = 1", 1, 1, 1, 11),
    "i3_otile_m1": lambda n: _project_case(n, "I = 3 (scalar loads), O = o_tile - 1, B = 2", 2, O_TILE - 1, 3, 12),
    "i2047_otile_p1": lambda n: _project_case(n, "I = slice - 1, O = o_tile + 1", 1, O_TILE + 1, I_SLICE - 1, 13, bias=False),
    "i2048_otile_b33": lambda n: _project_case(n, "I = slice (float4 loads), O = o_tile, B = b_tile + 1", B_TILE + 1, O_TILE, I_SLICE, 14),
    "i2048_unaligned": lambda n: _project_case(n, "I = slice with an unaligned row base: scalar loads", 2, 5, I_SLICE, 15, unaligned=True),
    "i2049_o3": lambda n: _project_case(n, "I = slice + 1: a second slice of one column", 2, 3, I_SLICE + 1, 16),
    "i4100_b32": lambda n: _project_case(n, "I = 2 slice + 4 (float4 loads, three slices), B = b_tile", B_TILE, 5, 2 * I_SLICE + 4, 17),
    # the edges of the staging the projection shares with retrieval (csrc/mfma_tile.h): a row tail of either operand at every I
    "i36_o129_b33": lambda n: _project_case(n, "I = a chunk and one float4 (float4 loads), O = o_tile + 1, B = b_tile + 1", B_TILE + 1,
                                            O_TILE + 1, 36, 18),
    "i33_o129_b33": lambda n: _project_case(n, "I = a chunk and one float (scalar loads), O = o_tile + 1, B = b_tile + 1", B_TILE + 1,
                                            O_TILE + 1, 33, 19),
    "i2084_o129_b33": lambda n: _project_case(n, "I = slice + 36: the chunk and the float4 behind a slice edge", B_TILE + 1, O_TILE + 1,
                                              I_SLICE + 36, 20),
    # the exact family
    "exact_k4": lambda n: exact_case(n, "exact: K = 4, N = T + 6, D = 8, O = 3, constant score bias", 2, 8, 4, T + 6, 3, 21, True),
    "exact_k64": lambda n: exact_case(n, "exact: K = 64, D = d_tile + 1, N = 2 T + 1, no biases", 1, D_TILE + 1, 64, 2 * T + 1, 2, 22, False),
    "exact_i4100": lambda n: exact_project_case(n, "exact: I = 2 slice + 4, O = o_tile + 1, B = b_tile + 1", B_TILE + 1, O_TILE + 1, 2 * I_SLICE + 4, 23),
    "exact_i2049_unaligned": lambda n: exact_project_case(n, "exact: I = slice + 1, unaligned", 2, 3, I_SLICE + 1, 24, unaligned=True),
}
HEAD_CASES = sorted(n for n in CASES if not n.startswith(("i", "exact_i")))
PROJECT_CASES = sorted(n for n in CASES if n.startswith(("i", "exact_i")))
EXACT_CASES = sorted(n for n in CASES if n.startswith("exact"))


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case: float32 CPU tensors, shared, never modified"""
    return CASES[name](name)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    return oracle_chain(case(name))


def retrieval_margin(name="retrieval"):
    """(oracle indices [Q, k], smallest gap between adjacent similarities of a query's top-(k + 1), descriptor bar): the bar of a
    similarity of unit descriptors is the sum of the two descriptors' bars in the 2-norm, taken at its largest over the rows"""
    c = case(name)
    o = oracle_of(name)
    y, bar = o["y"], o["y_bar"]
    db, q = y[:c["n_db"]], y[c["n_db"]:]
    sims = q @ db.t()
    top, idx = sims.sort(1, descending=True)
    gap = float((top[:, :c["topk"]] - top[:, 1:c["topk"] + 1]).min())
    desc_bar = 2.0 * float(bar.pow(2).sum(1).sqrt().max())
    return idx[:, :c["topk"]], gap, desc_bar
