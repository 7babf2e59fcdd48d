"""References and named cases of the grid-encoding tests (tests/test_gpu_grid_encoding.py, tests/test_gpu_grid_encoding_edges.py,
tests/test_host_grid_encoding_edges.py).

* `restated`: the float64 torch restatement of the encoding (any device), differentiable in the table and in the points.
* `float64_reference`: everything the tests compare against, from `restated` and autograd: outputs, both gradients and the
  sums of |terms| that scale the three bars.
* `model32`: a float32 numpy model of the kernels as written (csrc/grid_encoding.hip, grid_encoding.h), with one deliberate
  defect per name of `WRONG`.  It runs on the CPU and shows that the checks are reachable by a correct f32 implementation and
  fail for a wrong one.
* Named layouts (`EXACT`, `BOUNDED`) and seeded point builders, each with the edge it exists for.

The exact family: per_level_scale 2 and an integer base resolution make every scale base * 2^l - 1 an integer.  With points in
eighths, integer table entries and integer upstream gradients, pos, frac, every weight (a multiple of 2^-9), every product and
every partial sum are exact in float32, so the forward, the table gradient in any order of its atomics and the input gradient
equal the float64 restatement bit for bit.  `EXACT_TERMS_BELOW` / `EXACT_DX_BELOW` are the magnitudes that keep it so."""
import functools

import numpy as np
import torch

M32 = 0xFFFFFFFF
PRIMES = (1, 2654435761, 805459861)

EXACT_N = 2048
EXACT_TERMS_BELOW = 2.0 ** 13          # sum of |terms| per table entry, terms being multiples of 2^-9: 22 bits
EXACT_DX_BELOW = 2.0 ** 15             # bound of the input-gradient terms, multiples of 2^-6: 21 bits


def restated(x, params, lay, want_x_grad=False, G=None):
    """out [N, L*F] (float64) of the grid encoding, plus the per-element sum of |terms|.  `x` f32 [N, D]; `params` [n_params]
    (any float dtype, may require grad).  With want_x_grad, `x` must be float64 requiring grad: its value must be f32-exact;
    the cell and frac come from the f32 arithmetic, frac's derivative is scale.  With G (dL/dout), a third result [N, 1]:
    sum over levels of scale * sum over corners |<G, corner feature>|, which bounds every term of dL/dx."""
    D, F = lay.n_input_dims, lay.n_features_per_level
    x32 = x.detach().float()
    outs, abss = [], []
    xbound = torch.zeros((x.shape[0], 1), dtype=torch.float64, device=x.device)
    for lvl in range(lay.n_levels):
        scale, res, size, off = lay.scales[lvl], lay.resolutions[lvl], lay.sizes[lvl], lay.offsets[lvl]
        pos = (x32.double() * scale + 0.5).float()          # fmaf(scale, x, 0.5f): exact in f64, rounded to f32 once
        fl = torch.floor(pos)
        cell = fl.to(torch.int64) & M32
        frac = (pos - fl).double()
        if want_x_grad:
            frac = frac + (x - x.detach()) * scale
        acc = torch.zeros((x.shape[0], F), dtype=torch.float64, device=x.device)
        sabs = torch.zeros_like(acc)
        for c in range(1 << D):
            g = [(cell[:, d] + ((c >> d) & 1)) & M32 for d in range(D)]
            stride, index = 1, torch.zeros_like(g[0])
            for d in range(D):
                if stride <= size:
                    index = (index + g[d] * stride) & M32
                    stride = stride * res & M32
            if lay.grid_type == 0 and size < stride:
                index = torch.zeros_like(g[0])
                for d in range(D):
                    index = index ^ ((g[d] * PRIMES[d]) & M32)
            index = index % size
            w = torch.ones_like(frac[:, 0])
            for d in range(D):
                w = w * (frac[:, d] if (c >> d) & 1 else 1.0 - frac[:, d])
            rows = (off + index)[:, None] * F + torch.arange(F, device=x.device)[None, :]
            v = params.double()[rows]
            acc = acc + w[:, None] * v
            sabs = sabs + (w[:, None] * v).abs().detach()
            if G is not None:
                xbound += scale * (G[:, lvl * F:(lvl + 1) * F].double() * v.detach()).sum(1, keepdim=True).abs()
        outs.append(acc)
        abss.append(sabs)
    if G is not None:
        return torch.cat(outs, 1), torch.cat(abss, 1), xbound
    return torch.cat(outs, 1), torch.cat(abss, 1)


def float64_reference(x, params, lay, G):
    """what the tests compare against, on the device of `x`: out, dparams and dx of sum(out * G) in float64, with out_abs (sum of
    |terms| per output), dparams_abs (sum of |terms| per table entry: the weights are >= 0) and dx_bound [N, 1].  On a cell face
    the cell is fixed by floorf of the f32 pos, so dx is the right-hand derivative there."""
    x64 = x.detach().double().requires_grad_(True)
    p64 = params.detach().double().requires_grad_(True)
    out, out_abs, dx_bound = restated(x64, p64, lay, want_x_grad=True, G=G)
    (out * G.double()).sum().backward()
    p_abs = p64.detach().clone().requires_grad_(True)
    ref_abs, _ = restated(x.detach(), p_abs, lay)
    (ref_abs * G.double().abs()).sum().backward()
    return {"out": out.detach(), "out_abs": out_abs, "dparams": p64.grad, "dparams_abs": p_abs.grad, "dx": x64.grad,
            "dx_bound": dx_bound}


def _worst(err, bar):
    """largest err / bar; wherever `err <= bar` does not hold and the ratio does not say so itself (an error where the bar is 0,
    a NaN or infinite error) it counts as infinite, so the result is never NaN and `<= 1` means `(err <= bar).all()`"""
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    told = torch.isfinite(r) & (r > 1.0)
    r = torch.where((err <= bar) | told, r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def within(r):
    """every ratio of `ratios` at most 1 (a NaN would fail, though `_worst` gives none)"""
    return all(v <= 1.0 for v in r.values())


def ratios(got, ref):
    """worst |got - float64| / bar of each of `out`, `dparams`, `dx` present in `got`, under the project's three bars: forward
    4 * 2^-23 * sum|terms|, table gradient 1e-5 * sum|terms| per entry (exactly 0 where nothing contributes: a nonzero there is
    inf), input gradient 1e-5 * bound"""
    r = {}
    if "out" in got:
        r["out"] = _worst((got["out"].double() - ref["out"]).abs(), 4 * 2.0 ** -23 * ref["out_abs"])
    if "dparams" in got:
        r["dparams"] = _worst((got["dparams"].double() - ref["dparams"]).abs(), 1e-5 * ref["dparams_abs"])
    if "dx" in got:
        r["dx"] = _worst((got["dx"].double() - ref["dx"]).abs(), 1e-5 * ref["dx_bound"].expand_as(ref["dx"]))
    return r


def inexact(got, ref):
    """names among `out`, `dparams`, `dx` in `got` whose values are not the float64 ones"""
    return [k for k in ("out", "dparams", "dx") if k in got and not torch.equal(got[k].double(), ref[k])]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- named layouts ---------------------------------------------------------------------------------------------------

def _grid(kind, L, F, base, pls, log2_T=19):
    return {"otype": "Grid", "type": kind, "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2_T,
            "base_resolution": base, "per_level_scale": pls}


# name: (D, configuration, the edge it exists for)
EXACT = {}
for _D in (2, 3):
    for _F in (1, 2, 4, 8):
        EXACT[f"int6_hash_d{_D}f{_F}"] = (_D, _grid("Hash", 6, _F, 1, 2.0, 8 if _D == 3 else 4),
                                          "8 lanes per point, 6 live; levels 0-2 dense, 3-5 hashed; level 0 has scale 0, resolution 1")
        EXACT[f"int6_dense_d{_D}f{_F}"] = (_D, _grid("Dense", 6, _F, 1, 2.0), "the dense index of every level, scale 0 at level 0")
        EXACT[f"int6_tiled_d{_D}f{_F}"] = (_D, _grid("Tiled", 6, _F, 1, 2.0),
                                           "one entry per level: every corner of every point adds to the same entry")
EXACT["eq3"] = (3, _grid("Hash", 3, 4, 4, 2.0, 4), "level 0: resolution 4, size 16, the stride equals the size after two dimensions")
EXACT["eq2"] = (2, _grid("Hash", 3, 1, 8, 2.0, 3), "level 0: resolution 8 = size, the stride equals the size after one dimension")

BOUNDED = {
    "one_level": (3, _grid("Dense", 1, 4, 17, 2.0), "one lane per point: no shuffle step, every lane is level 0"),
    "two": (2, _grid("Hash", 2, 2, 16, 1.5, 8), "two lanes per point, (D, F) = (2, 2)"),
    "three": (3, _grid("Dense", 3, 8, 3, 1.7), "four lanes per point, one idle; dense in three dimensions at F = 8"),
    "tiled5": (3, _grid("Tiled", 4, 2, 5, 1.7), "sizes of 125, odd level offsets 125, 250, 375; the stride passes the size mid-loop"),
    "tiled5_2": (2, _grid("Tiled", 4, 2, 5, 1.7), "tiled in two dimensions, sizes of 25"),
    "L17": (2, _grid("Dense", 17, 1, 2, 1.25), "32 lanes per point, 15 of them idle but part of the shuffle sum"),
    "L32": (3, _grid("Hash", 32, 8, 2, 1.2, 10), "the maximum: two points per wave, rows of 256 floats"),
    "flat": (2, _grid("Dense", 3, 2, 7, 1.0), "per_level_scale 1: three identical levels"),
    "shrinking": (3, _grid("Hash", 5, 1, 16, 0.8, 9), "per_level_scale below 1: resolutions fall with the level"),
}
LAYOUTS = {**EXACT, **BOUNDED}


@functools.lru_cache(maxsize=None)
def layout(name):
    """the host level table of a named layout; an exact layout asserts, from its own scales, that they are integers"""
    from splatloc_amd.grid_encoding import GridLayout
    D, cfg, _ = LAYOUTS[name]
    lay = GridLayout(D, cfg)
    if name in EXACT:
        assert all(float(s).is_integer() and 0 <= s < 64 for s in lay.scales), (name, lay.scales)
    return lay


def lanes_per_point(lay):
    lp = 1
    while lp < lay.n_levels:
        lp *= 2
    return lp


def hashed_levels(lay):
    """per level: is it indexed by the hash (Hash grids only: the dense grid outgrows the size)"""
    return [lay.grid_type == 0 and r ** lay.n_input_dims > s for r, s in zip(lay.resolutions, lay.sizes)]


def stride_meets_size(lay, lvl):
    """does the stride of corner_index equal the level's size after some dimension (where `<=` and `<` part ways)"""
    return any(lay.resolutions[lvl] ** d == lay.sizes[lvl] for d in range(1, lay.n_input_dims))


def batch_sizes(lay):
    """the last point of a workgroup of 256 lanes, the first of the next, a partial last wave"""
    per_group = 256 // lanes_per_point(lay)
    return [1, per_group - 1, per_group, per_group + 1, 777]


# ---- seeded values ---------------------------------------------------------------------------------------------------

def points(n, seed, lay):
    """uniform points plus points on cell faces (pos = scale x + 0.5 an integer, up to the f32 rounding of x) of every level,
    at 0 and 1, and a few outside [0, 1]"""
    D = lay.n_input_dims
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, D), generator=g)
    if n >= 64:
        k = n // 8
        lvl = torch.randint(0, lay.n_levels, (k, D), generator=g)
        scale = torch.tensor(lay.scales, dtype=torch.float64)[lvl]
        x[:k] = ((torch.floor(x[:k].double() * scale) + 0.5) / scale).float()
        x[k:2 * k, 0] = 0.0
        x[2 * k:3 * k, 1] = 1.0
        x[3 * k:3 * k + 8] = torch.tensor([[-0.25, 0.5, 1.5], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 2.0, 0.5],
                                           [0.5, -0.01, 1.01], [1.25, 0.75, -0.5], [0.0, 1.0, 0.0], [3.0, -2.0, 0.25]])[:, :D]
    return x


SMALL_POOL = 512


def bounded_points(n, seed, lay):
    """`points`; below 64 rows, where its face recipe does not apply, rows of a draw of 512 taken in turn from its face rows, its
    outside rows, its rows at 0, its rows at 1 and its uniform rows, so that a batch of 7 still holds each kind"""
    if n >= 64:
        return points(n, seed, lay)
    pool = points(SMALL_POOL, seed, lay)
    k = SMALL_POOL // 8
    starts = (0, 3 * k, k, 2 * k, 3 * k + 8)
    return pool[[starts[i % 5] + i // 5 for i in range(n)]].clone()


def exact_points(n, seed, lay):
    """multiples of 1/8 in [-1, 2]: faces (frac 0), negative cells, 0 and 1 all occur, and pos is exact at integer scales"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 17, (n, lay.n_input_dims), generator=g).float() / 8


def exact_table(seed, lay):
    """integers in [-8, 8]"""
    return torch.randint(-8, 9, (lay.n_params,), generator=torch.Generator().manual_seed(seed)).float()


def exact_grad(n, seed, lay):
    """integers in [-4, 4]"""
    return torch.randint(-4, 5, (n, lay.n_output_dims), generator=torch.Generator().manual_seed(seed)).float()


def table(seed, lay):
    """uniform(-1, 1): values that mean something"""
    return torch.rand((lay.n_params,), generator=torch.Generator().manual_seed(seed)) * 2 - 1


def grad(n, seed, lay):
    return torch.randn((n, lay.n_output_dims), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def exact_case(name, n=EXACT_N):
    """(x, table, dL/dout) of an exact layout, on the CPU; shared, never modified.  The seeds are a draw for which the float64
    restatement keeps both magnitude conditions on every exact layout (the one-entry tables at D = 3, F = 8, where no two
    corners cancel, pass 2^15 on most draws; exactness itself has 2^3 to spare beyond that).  A change of these seeds may
    therefore trip the 2^15 assertion of test_exact_family_stays_exact for int6_tiled_d3f8 although nothing has gone wrong: draw
    again until the restatement keeps both conditions, and leave the value ranges and the two conditions as they are."""
    lay = layout(name)
    return exact_points(n, 401, lay), exact_table(402, lay), exact_grad(n, 403, lay)


@functools.lru_cache(maxsize=None)
def bounded_case(name, n):
    """(x, table, dL/dout) of a bounded layout at batch size n, on the CPU; shared, never modified"""
    lay = layout(name)
    return bounded_points(n, 211 + n, lay), table(212, lay), grad(n, 213 + n, lay)


def case(name, n=None):
    return exact_case(name, n or EXACT_N) if name in EXACT else bounded_case(name, n)


@functools.lru_cache(maxsize=None)
def reference(name, n=None, device="cpu"):
    """float64_reference of case(name, n), computed once per device and shared"""
    x, p, G = (t.to(device) for t in case(name, n))
    return float64_reference(x, p, layout(name), G)


# ---- the checks, written once for the device and for model32 ---------------------------------------------------------
# `run(x, params, lay, G, want)` evaluates the encoding on tensors of one device and returns a dict of f32 tensors there.

ROWS_N = 777
ROWS_LAYOUTS = ("int6_hash_d3f2", "L17", "L32")
COLLISION_LAYOUTS = ("int6_tiled_d3f2", "int6_tiled_d2f8", "eq2")
COLLISION_NS = (2, 16, 256, 2048)


def check_exact(run, name, device="cpu", want=("out", "dparams", "dx")):
    """names whose values differ from the float64 restatement on an exact case"""
    x, p, G = (t.to(device) for t in case(name))
    return inexact(run(x, p, layout(name), G, want), reference(name, None, device))


def check_bounded(run, name, n, device="cpu"):
    """worst ratio against each of the three bars on a bounded case"""
    x, p, G = (t.to(device) for t in case(name, n))
    return ratios(run(x, p, layout(name), G, ("out", "dparams", "dx")), reference(name, n, device))


def check_rows(run, name, device="cpu", sample=100):
    """a point's row depends on nothing but the point: rows of a batch of 777 against one-point batches, and the input gradient of
    the batch against that of a fixed permutation of it, bit for bit; the failures by name"""
    lay = layout(name)
    x, p, G = (t.to(device) for t in case(name, ROWS_N))
    full = run(x, p, lay, G, ("out", "dx"))
    g = torch.Generator().manual_seed(5)
    failed = []
    for i in torch.randperm(ROWS_N, generator=g)[:sample].tolist():
        if not same_bits(run(x[i:i + 1], p, lay, None, ("out",))["out"][0], full["out"][i]):
            failed.append(f"row {i} alone")
    perm = torch.randperm(ROWS_N, generator=g).to(device)
    again = run(x[perm], p, lay, G[perm], ("out", "dx"))
    if not same_bits(again["out"], full["out"][perm]):
        failed.append("out permuted")
    if not same_bits(again["dx"], full["dx"][perm]):
        failed.append("dx permuted")
    return failed


def check_collisions(run, name, device="cpu"):
    """N copies of one point give exactly N times the point's table gradient (N a power of two, exact values): the N for which
    they do not"""
    lay = layout(name)
    x, p, G = (t.to(device) for t in case(name))
    one = run(x[:1], p, lay, G[:1], ("dparams",))["dparams"]
    assert float(one.abs().sum()) > 0
    return [n for n in COLLISION_NS
            if not torch.equal(run(x[:1].expand(n, -1).contiguous(), p, lay, G[:1].expand(n, -1).contiguous(), ("dparams",))["dparams"],
                               n * one)]


def cell_census(x, lay):
    """per level: (rows with a frac of exactly 0, rows with a negative cell, is every pos = scale * x + 0.5 exact in f32)"""
    x64 = x.double()
    rows = []
    for scale in lay.scales:
        exact = x64 * scale + 0.5
        pos = exact.float()
        fl = torch.floor(pos)
        rows.append((int(((pos - fl) == 0).any(1).sum()), int((fl < 0).any(1).sum()), bool((pos.double() == exact).all())))
    return rows


# ---- the float32 model of the kernels --------------------------------------------------------------------------------

# deliberate defects of model32: name -> what is wrong
WRONG = {
    "stride_lt": "the stride test of corner_index is `<`, not `<=`",
    "hash_le": "a level is hashed when size <= stride",
    "primes_swapped": "the primes of dimensions 0 and 1 swapped",
    "no_wrap": "the index formed in int64, without the uint32 wrap before % size",
    "trunc": "pos truncated towards zero instead of floorf",
    "no_half": "the + 0.5 of pos dropped",
    "clamp": "x clamped to [0, 1]",
    "weight_swapped": "frac and 1 - frac exchanged in the corner weight",
    "corner_bit_reversed": "corner bit d moves the cell of dimension D-1-d (the weights keep their dimension)",
    "feature_major": "output and gradient columns feature-major (f * L + level)",
    "offset_no_F": "the level offset not multiplied by F",
    "first4": "only the first four features of an F = 8 entry and gradient row used",
    "dx_sign": "the input gradient's sign flipped",
    "dx_no_scale": "the input gradient's scale factor dropped",
    "dx_pow2_levels": "the input gradient summed over the first 2^floor(log2 L) levels only",
    "dx_2lp": "the input gradient summed over 2 * Lp lanes: the neighbouring point leaks in",
    "dp_store": "the table gradient stored instead of added",
}


def _fma32(a, b, c):
    """fmaf on f32 arrays: the product of two f32 is exact in f64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def model32(x, params, lay, G=None, want=("out", "dparams", "dx"), wrong=None):
    """The kernels as written, in float32 on the CPU: pos = fmaf(scale, x, 0.5f), floorf, uint32 cells; the output an fmaf chain
    in corner order; weights products in dimension order; the table gradient w * g added entry by entry (point order); the
    derivative weight +-scale times the other dimensions' factors, fmaf'd in corner order per level and summed over the point's
    Lp lanes by halving (what lane 0 holds after the xor shuffles).  Returns a dict of f32 CPU tensors of the names in `want`
    (`dparams` and `dx` need G).  `wrong` names one defect of WRONG."""
    assert wrong is None or wrong in WRONG, wrong
    f32 = np.float32
    D, F, L = lay.n_input_dims, lay.n_features_per_level, lay.n_levels
    xs = x.detach().cpu().numpy().astype(f32)
    if wrong == "clamp":
        xs = np.clip(xs, f32(0), f32(1))
    p = params.detach().cpu().numpy().astype(f32)
    g = None if G is None else G.detach().cpu().numpy().astype(f32)
    want = [k for k in want if k == "out" or g is not None]
    N, Lp = xs.shape[0], lanes_per_point(lay)
    out = np.zeros((N, L * F), f32)
    dp = np.zeros_like(p)
    gx = np.zeros((N, Lp, D), f32)
    primes = (PRIMES[1], PRIMES[0], PRIMES[2]) if wrong == "primes_swapped" else PRIMES
    wrap = (lambda a: a) if wrong == "no_wrap" else (lambda a: a & M32)
    used = 4 if wrong == "first4" and F == 8 else F
    one = f32(1)
    for lvl in range(L):
        scale, res, size, off = f32(lay.scales[lvl]), lay.resolutions[lvl], lay.sizes[lvl], lay.offsets[lvl]
        pos = (xs.astype(np.float64) * float(scale) + (0.0 if wrong == "no_half" else 0.5)).astype(f32)
        fl = np.trunc(pos) if wrong == "trunc" else np.floor(pos)
        cell = fl.astype(np.int64)
        frac = (pos - fl).astype(f32)
        cols = np.array([f * L + lvl if wrong == "feature_major" else lvl * F + f for f in range(F)])
        base = off if wrong == "offset_no_F" else off * F
        gl = None
        if g is not None:
            gl = g[:, cols].copy()
            gl[:, used:] = 0
        acc = np.zeros((N, F), f32)
        for c in range(1 << D):
            bits = [(c >> d) & 1 for d in range(D)]
            ibits = bits[::-1] if wrong == "corner_bit_reversed" else bits
            gc = [wrap(cell[:, d] + ibits[d]) for d in range(D)]
            stride, index = 1, np.zeros((N,), np.int64)
            for d in range(D):
                if (stride < size) if wrong == "stride_lt" else (stride <= size):
                    index = wrap(index + gc[d] * stride)
                    stride = wrap(stride * res)
            if lay.grid_type == 0 and ((size <= stride) if wrong == "hash_le" else (size < stride)):
                index = np.zeros((N,), np.int64)
                for d in range(D):
                    index = index ^ wrap(gc[d] * primes[d])
            index = index % size
            fac = [(one - frac[:, d], frac[:, d]) for d in range(D)]
            if wrong == "weight_swapped":
                fac = [(b, a) for a, b in fac]
            w = np.ones((N,), f32)
            for d in range(D):
                w = w * fac[d][bits[d]]
            entry = (base + index * F)[:, None] + np.arange(F)[None, :]
            v = p[entry]
            v[:, used:] = 0
            if "out" in want:
                for f in range(F):
                    acc[:, f] = _fma32(w, v[:, f], acc[:, f])
            if "dparams" in want:
                vals = w[:, None] * gl
                if wrong == "dp_store":
                    dp[entry[:, :used].ravel()] = vals[:, :used].ravel()
                else:
                    np.add.at(dp, entry[:, :used].ravel(), vals[:, :used].ravel())
            if "dx" in want:
                dot = np.zeros((N,), f32)
                for f in range(F):
                    dot = _fma32(gl[:, f], v[:, f], dot)
                for d in range(D):
                    s = one if wrong == "dx_no_scale" else scale
                    wd = np.full((N,), s if bits[d] else -s, f32)
                    for e in range(D):
                        if e != d:
                            wd = wd * fac[e][bits[e]]
                    gx[:, lvl, d] = _fma32(wd, dot, gx[:, lvl, d])
        out[:, cols] = acc
    res_ = {}
    if "out" in want:
        res_["out"] = torch.from_numpy(out)
    if "dparams" in want:
        res_["dparams"] = torch.from_numpy(dp)
    if "dx" in want:
        if wrong == "dx_pow2_levels":
            keep = 1
            while keep * 2 <= L:
                keep *= 2
            gx[:, keep:] = 0
        m = Lp >> 1
        while m >= 1:
            gx = gx[:, :m] + gx[:, m:2 * m]
            m >>= 1
        dx = gx[:, 0]
        if wrong == "dx_2lp" and 2 * Lp <= 64:
            padded = np.concatenate([dx, np.zeros((N % 2, D), f32)])
            dx = (padded + padded.reshape(-1, 2, D)[:, ::-1].reshape(-1, D))[:N]
        if wrong == "dx_sign":
            dx = -dx
        res_["dx"] = torch.from_numpy(np.ascontiguousarray(dx))
    return res_
