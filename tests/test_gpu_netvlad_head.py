"""The device NetVLAD head (splatloc_amd/netvlad.py, csrc/netvlad_head.hip) against tests/netvlad_reference.py.

Every stage runs through its C entry into sentinel-filled buffers with a guard behind them, on the DEVICE'S OWN output of the
stage before, and is held to the float64 oracle of that input: aggregate and project within the derived elementwise bars, assign
and inv_norm within four times the restatement's own error on the case (tests/netvlad_reference.py has the derivations).  The exact
family is held bit for bit.  Rows are bit-identical for B = 1 and B = b_tile + 1 and from run to run; NetVLADHead.__call__ is
bit-identical to the staged calls and feeds localize.retrieve.

Measured on the MI355X, error / bar (the bound is 1; for assign and inv_norm 1 means four times the restatement's error):
  assign     n1_d3_k2 0.864 (the worst: one location, two clusters), layer 0.453, n129_d1_k2 0.391, no_whitening 0.345,
             n63_d31_k63 0.323, zero_locations 0.273, b32_d3_k2 0.269, n64_d32_k64 0.261, saturated and zero_image 0.250 (the
             restatement's own error), retrieval 0.198; 0 on n65_d33_k1 (K = 1) and the exact family
  inv_norm   0.076 (layer) to 0.256 (b32_d3_k2); 0.250 where the maximum errors coincide with torch's; 0 on the exact family
  raw V      b32_d3_k2 0.254, n1_d3_k2 0.231, no_whitening 0.074, n63_d31_k63 0.052, n64_d32_k64 0.047, retrieval 0.044, the
             others below 0.025, layer 0.004; 0 on the exact family
  v          b32_d3_k2 0.086, no_whitening 0.041, n1_d3_k2 0.033, the others below 0.025
  y raw      i3_otile_m1 0.348 (three terms), b32_d3_k2 0.183, i36_o129_b33 0.084, i33_o129_b33 0.078, zero_image 0.045,
             n65_d33_k1 0.041, n1_d3_k2 0.038, the others below 0.03; the 2048-, 2084- and 4100-column cases below 0.002; 0 on the
             exact family
  y          b32_d3_k2 0.056, i33_o129_b33 0.045, i36_o129_b33 0.035, i3_otile_m1 0.028, the others below 0.02
"""
import ctypes as C
import functools

import pytest
import torch

from splatloc_amd import _native, localize, netvlad as NV
from splatloc_amd._host import _stream
from tests import netvlad_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD          # a NaN no kernel computes
GUARD = 256


class _Out:
    """a float32 device buffer of `shape` filled with the sentinel, `lead` floats in front of it and a guard behind it"""

    def __init__(self, *shape, lead=0):
        self.n = 1
        for s in shape:
            self.n *= s
        self.lead = lead
        self.flat = torch.full((lead + self.n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.flat[lead:lead + self.n].view(*shape)

    def done(self):
        """everything inside written, nothing outside touched"""
        bits = self.flat.view(torch.int32)
        assert bool((bits[:self.lead] == SENTINEL).all()) and bool((bits[self.lead + self.n:] == SENTINEL).all()), "stored outside the output"
        assert not bool((bits[self.lead:self.lead + self.n] == SENTINEL).any()), "an element was never written"
        return self.t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ws(B, D, K, N, O):
    nb = C.c_size_t(0)
    assert _native.load().splatraster_netvlad_workspace_size(B, D, K, N, O, C.byref(nb)) == 0
    return torch.empty(max(nb.value, 1), dtype=torch.uint8, device="cuda"), nb.value


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def run_assign(x, w, b):
    B, D, N = x.shape
    K = w.shape[0]
    a, inv = _Out(B, K, N), _Out(B, N)
    st = _native.load().splatraster_netvlad_assign(B, D, K, N, _p(x), _p(w), _p(b), _p(a.t), _p(inv.t), None, 0, _stream(x.device))
    assert st == 0
    return a.done(), inv.done()


def run_aggregate(x, a, inv, centers, flags):
    B, D, N = x.shape
    K = a.shape[1]
    v = _Out(B, D * K)
    st = _native.load().splatraster_netvlad_aggregate(B, D, K, N, _p(x), _p(a), _p(inv), _p(centers), flags, _p(v.t), None, 0,
                                                      _stream(x.device))
    assert st == 0
    return v.done()


def run_project(x, weight, bias, flags, partial=False):
    """`weight` as given: the caller decides its alignment.  partial: also the slices' raw sums [slices][B][O], the workspace's
    only section"""
    B, I = x.shape
    O = weight.shape[0]
    ws, nbytes = _ws(B, I, 1, 1, O)
    y = _Out(B, O)
    st = _native.load().splatraster_netvlad_project(B, O, I, _p(x), _p(weight), _p(bias), flags, _p(y.t), _p(ws), nbytes, _stream(x.device))
    assert st == 0
    if partial:
        slices = (I + R.I_SLICE - 1) // R.I_SLICE
        return y.done(), ws[:slices * B * O * 4].view(torch.float32).view(slices, B, O)
    return y.done()


def _shifted(w):
    """`w` on the device, one float into its buffer: only scalar loads can read it"""
    flat = torch.empty(w.numel() + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(w.shape)
    view.copy_(w)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _weight(c):
    w = c["whiten_w"]
    return _shifted(w) if c.get("unaligned") else w.cuda().contiguous()


@functools.lru_cache(maxsize=None)
def device_run(name):
    """the staged device run of a case, every stage on the device's own output of the one before: CPU tensors by the names of
    R.restatement"""
    c = R.case(name)
    out = {}
    if "features" in c:
        x, w, b, cen = _dev(c["features"]), _dev(c["score_w"]), _dev(c["score_b"]), _dev(c["centers"])
        a, inv = run_assign(x, w, b)
        raw = run_aggregate(x, a, inv, cen, 0)
        v = run_aggregate(x, a, inv, cen, R.flags_of(c))
        out.update(assign=a, inv_norm=inv, raw=raw, v=v)
    else:
        v = _dev(c["x"])
    if c.get("whiten_w") is not None:
        W, wb = _weight(c), _dev(c["whiten_b"])
        out["y_raw"] = run_project(v, W, wb, 0)
        out["y"] = run_project(v, W, wb, R.L2NORM)
        if "features" in c and c.get("exact"):
            out["raw_projected"] = run_project(out["raw"], W, wb, 0)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


def _head(c):
    return NV.NetVLADHead(_dev(c["score_w"]), _dev(c["centers"]), _dev(c["score_b"]), _dev(c["whiten_w"]), _dev(c["whiten_b"]),
                          c["intranorm"])


def test_the_cases_were_built_for_the_device_tiles():
    assert NV.tiles() == R.TILES


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_stage_within_its_bars(name):
    out = device_run(name)
    r = R.ratios(name, out)
    print(name, {k: round(v, 4) for k, v in r.items()})
    assert r and R.within(r), r


@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_family_bit_for_bit(name):
    c, out, o = R.case(name), device_run(name), R.oracle_of(name)
    for k in (("assign", "inv_norm", "raw") if "features" in c else ("y_raw",)):
        assert R.same_bits(out[k], o[k].float()), k
    if "features" in c:
        y = R.project64(out["raw"], c["whiten_w"], c["whiten_b"], 0)["y"]
        assert R.same_bits(out["raw_projected"], y.float())


def test_zero_locations_and_zero_image():
    c, out = R.case("zero_locations"), device_run("zero_locations")
    soft = torch.softmax(c["score_b"], 0)
    for b, n in c["zero"]:
        assert float(out["inv_norm"][b, n]) == float(torch.tensor(1.0) / torch.tensor(1e-12))
        assert float((out["assign"][b, :, n] - soft).abs().max()) <= 4e-7
    out = device_run("zero_image")
    assert bool(torch.isfinite(out["y"]).all()) and float(out["v"][1].norm()) == pytest.approx(1.0, abs=1e-5)


def test_saturated_logits_give_a_one_hot_assignment():
    out, o = device_run("saturated"), R.oracle_of("saturated")
    onehot = o["assign"][0].max(0).values == 1.0
    assert onehot.sum() >= 16
    a = out["assign"][0][:, onehot]
    assert bool(((a == 0) | (a == 1)).all()) and bool((a.sum(0) == 1).all())
    assert bool(torch.isfinite(out["assign"]).all())


def test_rows_do_not_depend_on_the_batch():
    """B = 1 against B = 46 > b_tile + 1: rows 0, b_tile and the last, every output bit for bit"""
    c, full = R.case("retrieval"), device_run("retrieval")
    assert c["features"].shape[0] > R.B_TILE + 1
    w, b, cen, W, wb = (_dev(c[k]) for k in ("score_w", "score_b", "centers", "whiten_w", "whiten_b"))
    for row in (0, R.B_TILE, c["features"].shape[0] - 1):
        x = c["features"][row:row + 1].cuda().contiguous()
        a, inv = run_assign(x, w, b)
        raw, v = run_aggregate(x, a, inv, cen, 0), run_aggregate(x, a, inv, cen, R.flags_of(c))
        one = {"assign": a, "inv_norm": inv, "raw": raw, "v": v, "y_raw": run_project(v, W, wb, 0), "y": run_project(v, W, wb, R.L2NORM)}
        for k, t in one.items():
            assert R.same_bits(t.cpu()[0], full[k][row]), (row, k)
    # the projection alone at B = b_tile + 1: the row behind the tile of images
    c, full = R.case("i2048_otile_b33"), device_run("i2048_otile_b33")
    W, wb = _weight(c), _dev(c["whiten_b"])
    for row in (0, R.B_TILE):
        y = run_project(c["x"][row:row + 1].cuda().contiguous(), W, wb, R.L2NORM)
        assert R.same_bits(y.cpu()[0], full["y"][row]), row


@pytest.mark.parametrize("name", ("retrieval", "n63_d31_k63", "i4100_b32"))
def test_repeat_runs_are_bit_identical(name):
    first = device_run(name)
    device_run.cache_clear()
    second = device_run(name)
    assert first is not second and first.keys() == second.keys()
    for k in first:
        assert R.same_bits(first[k], second[k]), k


@pytest.mark.parametrize("name", ("i36_o129_b33", "i2084_o129_b33"))
def test_float4_and_scalar_loads_project_the_same_bits(name):
    """the same numbers from 16-byte aligned buffers (I % 4 == 0: float4 loads) and through views one float into theirs (scalar
    loads): the slices' raw sums and y, bit for bit"""
    c = R.case(name)
    x, W, wb = _dev(c["x"]), _dev(c["whiten_w"]), _dev(c["whiten_b"])
    assert x.shape[1] % 4 == 0 and x.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    y4, p4 = run_project(x, W, wb, R.L2NORM, partial=True)
    y1, p1 = run_project(_shifted(c["x"]), _shifted(c["whiten_w"]), wb, R.L2NORM, partial=True)
    assert p4.shape[0] == (2 if name.startswith("i2084") else 1)
    assert R.same_bits(p4.cpu(), p1.cpu()) and R.same_bits(y4.cpu(), y1.cpu())
    assert R.same_bits(y4.cpu(), device_run(name)["y"])


@pytest.mark.parametrize("name", ("n63_d31_k63", "n65_d33_k1", "n129_d1_k2", "no_whitening", "zero_image"))
def test_call_is_the_staged_calls_bit_for_bit(name):
    c, out = R.case(name), device_run(name)
    head = _head(c)
    x = _dev(c["features"])
    y = head(x)
    want = out["y"] if c["whiten_w"] is not None else out["v"]
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape) and R.same_bits(y.cpu(), want)
    a, inv = head.assign(x)
    assert R.same_bits(a.cpu(), out["assign"]) and R.same_bits(inv.cpu(), out["inv_norm"])
    assert R.same_bits(head.vlad(x).cpu(), out["v"]) and R.same_bits(head.vlad(x, raw=True).cpu(), out["raw"])
    if c["whiten_w"] is not None:
        assert R.same_bits(head.project(head.vlad(x)).cpu(), out["y"])
    assert float((y.cpu().double().norm(dim=1) - 1).abs().max()) < 1e-5          # unit rows
    assert R.same_bits(head(x).cpu(), want)                                      # the cached workspace serves the next call


def test_four_dimensional_maps_and_state_dicts():
    c, out = R.case("n63_d31_k63"), device_run("n63_d31_k63")
    B, D, N = c["features"].shape
    sd = {"m.netvlad.score_proj.weight": c["score_w"][:, :, None], "m.netvlad.score_proj.bias": c["score_b"], "m.netvlad.centers": c["centers"],
          "m.whiten.weight": c["whiten_w"], "m.whiten.bias": c["whiten_b"]}
    head = NV.NetVLADHead.from_state_dict(sd, prefix="m.")
    assert (head.K, head.D, head.O) == (63, D, c["whiten_w"].shape[0])
    y = head(c["features"].reshape(B, D, 7, 9).cuda())
    assert R.same_bits(y.cpu(), out["y"])
    with pytest.raises(ValueError):
        head(torch.zeros(B, D + 1, N, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(c["features"])
    assert tuple(head(torch.zeros(0, D, N, device="cuda")).shape) == (0, head.O)


def test_call_feeds_retrieve_with_the_oracle_indices():
    c = R.case("retrieval")
    want, gap, bar = R.retrieval_margin()
    assert gap >= 64.0 * bar
    y = _head(c)(_dev(c["features"]))
    idx, sims = localize.retrieve(y[c["n_db"]:], y[:c["n_db"]], k=c["topk"])
    assert torch.equal(idx.cpu(), want)
    assert float((sims.cpu().double() - (R.oracle_of("retrieval")["y"][c["n_db"]:] @ R.oracle_of("retrieval")["y"][:c["n_db"]].t())
                  .gather(1, want)).abs().max()) <= 64.0 * bar
