"""tinycudann.Encoding on the MI355X at its variant, level and index edges (cases, references and checks:
tests/grid_encoding_reference.py; tests/test_host_grid_encoding_edges.py shows on a float32 model that these checks are
reachable and that each deliberate defect fails one of them).

* Exact family (26 layouts, N = 2048): forward, table gradient and input gradient equal the float64 restatement bit for bit, with
  both gradients, the table's alone and the input's alone, which launches all 8 forward and 24 backward instantiations; the
  backward twice gives the same bytes.
* Bounded family (9 layouts x 5 batch sizes around the workgroup boundary): the three bars of tests/test_gpu_grid_encoding.py,
  the input gradient on faces, at 0 and 1 and outside [0, 1] included (on a face the cell is fixed by floorf of the f32 pos,
  so the derivative is the right-hand one).
* Rows independent of their neighbours, collisions adding up, the wrapper's clone and cast paths, the C entry's accumulate and
  NULL contracts with guard regions.

Measured on the MI355X, worst |device - float64| / bar over a layout's five batch sizes (forward / table gradient / input
gradient): one_level 0.482 / 0.0187 / 0.00625, two 0.313 / 0.0181 / 0.00683, three 0.45 / 0.0263 / 0.00523, tiled5 0.465 /
0.0172 / 0.00334, tiled5_2 0.315 / 0.0153 / 0.0079, L17 0.323 / 0.0164 / 0.00472, L32 0.552 / 0.0254 / 0.00218, flat 0.329 /
0.0146 / 0.00839, shrinking 0.449 / 0.0193 / 0.00315.  Every exact case, isolation case and wrapper case bit for bit; no defect
found in the kernels or the wrapper."""
import ctypes as C
import functools

import pytest
import torch

from tests import grid_encoding_reference as R

pytestmark = pytest.mark.gpu


def _encoding(name, params):
    import tinycudann as tcnn
    D, cfg, _ = R.LAYOUTS[name]
    enc = tcnn.Encoding(D, cfg, dtype=torch.float)
    with torch.no_grad():
        enc.params.copy_(params.cuda())
    return enc


def _device(x, p, lay, G, want, name=None):
    """the `run` of the shared checks: the module's forward and autograd backward, asking for exactly the gradients in `want`"""
    enc = _encoding(name, p)
    enc.params.requires_grad_("dparams" in want)
    xg = x.clone().requires_grad_("dx" in want)
    out = enc(xg)
    got = {"out": out.detach()}
    if "dparams" in want or "dx" in want:
        out.backward(G)
        if "dparams" in want:
            got["dparams"] = enc.params.grad
        if "dx" in want:
            got["dx"] = xg.grad
    return got


def _run(name):
    return functools.partial(_device, name=name)


@pytest.mark.parametrize("name", list(R.EXACT))
def test_exact_family_bit_for_bit_in_every_direction(name):
    """every exact layout: the forward; the backward with both gradients (<PGRAD, XGRAD> = <true, true>), with the table's alone
    (<true, false>) and with the input's alone on a frozen table (<false, true>); the first of them twice, same bytes"""
    run = _run(name)
    assert R.check_exact(run, name, "cuda", ("out",)) == []
    assert R.check_exact(run, name, "cuda", ("out", "dparams", "dx")) == []
    assert R.check_exact(run, name, "cuda", ("out", "dparams")) == []
    assert R.check_exact(run, name, "cuda", ("out", "dx")) == []
    x, p, G = (t.cuda() for t in R.case(name))
    a, b = (run(x, p, R.layout(name), G, ("dparams", "dx")) for _ in range(2))
    assert all(R.same_bits(a[k], b[k]) for k in ("out", "dparams", "dx"))


@pytest.mark.parametrize("name", list(R.BOUNDED))
def test_bounded_family_within_the_three_bars(name):
    """forward within 4 * 2^-23 * sum|terms|, table gradient within 1e-5 * sum|terms| per entry and exactly 0 where nothing
    contributes, input gradient within 1e-5 * bound, at N = 1, the last point of a workgroup, the first of the next and 777, on
    uniform points, faces of every level, 0, 1 and outside points"""
    lay = R.layout(name)
    worst = {}
    for n in R.batch_sizes(lay):
        r = R.check_bounded(_run(name), name, n, "cuda")
        assert R.within(r), (name, n, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{name}: worst |device - float64| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("name", R.ROWS_LAYOUTS)
def test_rows_are_independent_of_their_neighbours(name):
    """row i of a batch of 777 equals the one-point batch of point i, the batch's dx equals that of a permutation of it row for
    row; with three rows replaced by NaN, inf and 1e30 and only x requiring grad, every other row keeps its bits (every index is
    taken % size, so those rows read inside the table; their own values are not asserted)"""
    run = _run(name)
    assert R.check_rows(run, name, "cuda") == []
    lay = R.layout(name)
    x, p, G = (t.cuda() for t in R.case(name, R.ROWS_N))
    clean = run(x, p, lay, G, ("dx",))
    assert bool(torch.isfinite(clean["out"]).all()) and bool(torch.isfinite(clean["dx"]).all())
    rows = [5, 300, 776]
    bad = x.clone()
    bad[rows[0], 0] = float("nan")
    bad[rows[0], 1] = 0.5
    bad[rows[1]] = float("inf")
    bad[rows[2]] = 1e30
    got = run(bad, p, lay, G, ("dx",))
    keep = torch.ones((R.ROWS_N,), dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert R.same_bits(got["out"][keep], clean["out"][keep]) and R.same_bits(got["dx"][keep], clean["dx"][keep])


@pytest.mark.parametrize("name", R.COLLISION_LAYOUTS)
def test_collisions_add_up(name):
    """N copies of one point: exactly N times one point's table gradient, N = 2 .. 2048; a lost or overwritten update is short"""
    assert R.check_collisions(_run(name), name, "cuda") == []


def _grads(enc, x, backward):
    enc.zero_grad()
    xg = x.clone().requires_grad_(True) if not x.requires_grad else x
    xg.grad = None
    out = enc(xg)
    backward(out)
    return out.detach(), enc.params.grad.clone(), xg.grad.clone()


def test_wrapper_takes_expanded_and_non_contiguous_gradients():
    """out.sum().backward() hands the wrapper a stride-0 gradient, G.t().contiguous().t() a column-major one: both give the bits
    of the contiguous call (exact layout, so the table gradient too)"""
    name = "int6_hash_d3f2"
    x, p, G = (t.cuda() for t in R.case(name))
    enc = _encoding(name, p)
    ones = torch.ones_like(G)
    want = _grads(enc, x, lambda out: out.backward(ones))
    got = _grads(enc, x, lambda out: out.sum().backward())
    assert all(R.same_bits(a, b) for a, b in zip(got, want)) and float(want[1].abs().sum()) > 0
    want = _grads(enc, x, lambda out: out.backward(G))
    Gt = G.t().contiguous().t()
    assert not Gt.is_contiguous() and torch.equal(Gt, G)
    got = _grads(enc, x, lambda out: out.backward(Gt))
    assert all(R.same_bits(a, b) for a, b in zip(got, want))
    assert R.inexact(dict(zip(("out", "dparams", "dx"), got)), R.reference(name, None, "cuda")) == []


@pytest.mark.parametrize("name", ["tiled5", "int6_hash_d3f1"])
def test_wrapper_clones_misaligned_views(name):
    """x = big[1:] (rows of 3 floats: 12 bytes off) and G a view one float into a flat buffer (a row of tiled5 is 8 floats, so a row
    offset alone would leave it aligned; int6 at F = 1 has rows of 6) put both off 16-byte alignment, so the wrapper's clone path
    runs in the forward and in the backward.  Output and dx keep the aligned call's bits; the table gradient, whose last bits
    follow the atomics' order, does so on the exact layout and meets its float64 bar on tiled5."""
    lay = R.layout(name)
    x, p, G = (t.cuda() for t in R.case(name, None if name in R.EXACT else 777))
    n = x.shape[0]
    enc = _encoding(name, p)
    want = _grads(enc, x, lambda out: out.backward(G))
    big_x = torch.zeros((n + 1, lay.n_input_dims), device="cuda")
    big_x[1:] = x
    big_g = torch.zeros((n * lay.n_output_dims + 1,), device="cuda")
    big_g[1:] = G.reshape(-1)
    xv, gv = big_x[1:], big_g[1:].view(n, lay.n_output_dims)
    assert xv.data_ptr() % 16 != 0 and gv.data_ptr() % 16 != 0 and xv.is_contiguous() and gv.is_contiguous()
    got = _grads(enc, xv.detach().requires_grad_(True), lambda out: out.backward(gv))
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[2], want[2])
    if name in R.EXACT:
        assert R.same_bits(got[1], want[1])
    ref = R.reference(name, None if name in R.EXACT else 777, "cuda")
    assert R.within(R.ratios(dict(zip(("out", "dparams", "dx"), got)), ref))


def test_wrapper_casts_float64_and_float16_inputs():
    """x in float64 or float16 on the device: cast to f32, the f32 call's output bits, dx cast back to the dtype of x"""
    name = "int6_hash_d3f2"
    x, p, G = (t.cuda() for t in R.case(name))
    enc = _encoding(name, p)
    want = _grads(enc, x, lambda out: out.backward(G))
    for dtype in (torch.float64, torch.float16):
        xd = x.to(dtype)
        assert torch.equal(xd.float(), x)                  # eighths in [-1, 2] are exact in both
        got = _grads(enc, xd.requires_grad_(True), lambda out: out.backward(G))
        assert got[0].dtype == torch.float32 and R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
        assert got[2].dtype == dtype and torch.equal(got[2], want[2].to(dtype))
    xb, pb, _ = (t.cuda() for t in R.case("L17", 777))
    encb = _encoding("L17", pb)
    with torch.no_grad():
        assert R.same_bits(encb(xb.half()), encb(xb.half().float())) and R.same_bits(encb(xb.double()), encb(xb))


# ---- the C entry through ctypes --------------------------------------------------------------------------------------

GUARD = 4096
SENTINEL = -77.0


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _c_backward(lay, n, x, p, G, dp, dx):
    from splatloc_amd import _native
    st = _native.load().splatraster_grid_encoding_backward(C.byref(lay.native), n, _ptr(x), _ptr(p), _ptr(G), _ptr(dp), _ptr(dx), None)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("name", ["int6_hash_d3f2", "int6_tiled_d2f8", "eq3"])
def test_c_backward_accumulates_and_stays_inside_its_buffers(name):
    """splatraster_grid_encoding_backward adds onto dL_dparams (pre-filled with integers: exact) and writes N rows of dL_dx and
    nothing after them.  With dL_dparams NULL the kernel without table atomics runs: the table-gradient buffer of the call
    before, still allocated, keeps its bytes and dL_dx is the same.  With both outputs NULL nothing is written: that buffer, a
    sentinel-filled dL_dx buffer of the call before and the inputs keep their bytes.  x, the table and dL/dout are unchanged
    after every call.  On the null stream."""
    lay = R.layout(name)
    x, p, G = (t.cuda() for t in R.case(name))
    kept = [t.clone() for t in (x, p, G)]
    n, D = x.shape
    ref = R.reference(name, None, "cuda")
    torch.cuda.synchronize()

    def inputs_unchanged():
        return all(R.same_bits(a, b) for a, b in zip((x, p, G), kept))

    pre = torch.randint(-16, 17, (lay.n_params + GUARD,), generator=torch.Generator().manual_seed(9)).float().cuda()
    dp = pre.clone()
    dx = torch.full((n * D + GUARD,), SENTINEL, device="cuda")
    assert _c_backward(lay, n, x, p, G, dp, dx) == 0
    assert torch.equal(dp[:lay.n_params].double(), pre[:lay.n_params].double() + ref["dparams"])
    assert torch.equal(dp[lay.n_params:], pre[lay.n_params:])
    assert torch.equal(dx[:n * D].view(n, D).double(), ref["dx"]) and bool((dx[n * D:] == SENTINEL).all()) and inputs_unchanged()
    assert _c_backward(lay, n, x, p, G, dp, None) == 0                                   # a second call adds again
    assert torch.equal(dp[:lay.n_params].double(), pre[:lay.n_params].double() + 2 * ref["dparams"])
    assert torch.equal(dp[lay.n_params:], pre[lay.n_params:]) and inputs_unchanged()
    twice = dp.clone()
    dx = torch.full((n * D + GUARD,), SENTINEL, device="cuda")
    assert _c_backward(lay, n, x, p, G, None, dx) == 0                                   # dL_dparams NULL
    assert torch.equal(dx[:n * D].view(n, D).double(), ref["dx"]) and bool((dx[n * D:] == SENTINEL).all())
    assert R.same_bits(dp, twice) and inputs_unchanged()
    m = 5                                                                                # fewer rows than the buffer holds
    dx = torch.full((n * D + GUARD,), SENTINEL, device="cuda")
    assert _c_backward(lay, m, x, p, G, None, dx) == 0
    assert torch.equal(dx[:m * D].view(m, D).double(), ref["dx"][:m]) and bool((dx[m * D:] == SENTINEL).all())
    assert R.same_bits(dp, twice) and inputs_unchanged()
    dx.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert _c_backward(lay, n, x, p, G, None, None) == 0                                 # both NULL
    assert bool((dx == SENTINEL).all()) and R.same_bits(dp, twice) and inputs_unchanged()


@pytest.mark.parametrize("name,n", [("int6_hash_d3f2", 2048), ("L32", 9), ("L17", 7), ("one_level", 257)])
def test_c_forward_writes_its_rows_and_nothing_after_them(name, n):
    from splatloc_amd import _native
    lay = R.layout(name)
    x, p, _ = (t.cuda() for t in R.case(name, n))
    ref = R.reference(name, n if name in R.BOUNDED else None, "cuda")
    width = lay.n_output_dims
    out = torch.full((n * width + GUARD,), SENTINEL, device="cuda")
    torch.cuda.synchronize()
    assert _native.load().splatraster_grid_encoding_forward(C.byref(lay.native), n, _ptr(x), _ptr(p), _ptr(out), None) == 0
    torch.cuda.synchronize()
    got = {"out": out[:n * width].view(n, width)}
    assert R.ratios(got, ref)["out"] <= 1.0 and bool((out[n * width:] == SENTINEL).all())
    if name in R.EXACT:
        assert R.inexact(got, ref) == []
