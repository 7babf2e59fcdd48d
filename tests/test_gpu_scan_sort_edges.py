"""The device-wide prefix sum and the stable radix sort (csrc/scan_sort.hip) against np.cumsum and a stable argsort, bit for bit,
at the tile, path and digit edges: every case of tests/scan_sort_reference.py through the C ABI's test hooks
(splatraster_debug_scan_u32, splatraster_sort_pairs_u32, splatraster_debug_sort_pairs_k16).  tests/test_host_scan_sort_edges.py
proves on the CPU that every case takes the path it names and that its data exposes the wrong model it is there for.  Needs an
MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scan_sort_reference as R

pytestmark = pytest.mark.gpu

U32 = np.uint32
DEV = "cuda:0"


def _lib():
    from splatloc_amd import _native
    return _native.load()


def _check(rc, what):
    from splatloc_amd import _native
    _native.check(rc, what)


def _dev(a):
    """a uint32 array as an int32 tensor on the device (a fresh copy)"""
    return torch.from_numpy(np.array(a, dtype=U32).view(np.int32)).to(DEV)


def _host(t):
    return t.cpu().numpy().view(U32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tmp(nbytes, poison):
    return torch.full((max(int(nbytes), 1),), 0xFF if poison else 0, dtype=torch.uint8, device=DEV)


# ---- scan ----------------------------------------------------------------------------------------------------------------------
def run_scan(values, perm, mode, tmp=None, poison=True, span=None):
    """one call of the scan hook on the current stream: (out, total, span_owner or None, tmp) as host arrays; `tmp` is reused when
    given and otherwise made, filled with 0xFF bytes (the call clears the state it needs itself)"""
    lib = _lib()
    n = len(values)
    exclusive = mode == "exclusive in place"
    d_in = _dev(values) if n else None
    d_perm = _dev(perm) if perm is not None else None
    d_out = d_in if mode != "inclusive" else torch.full((n,), 0x55555555, dtype=torch.int32, device=DEV)
    if n == 0:
        d_out = None
    d_total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    if tmp is None:
        tmp = _tmp(lib.splatraster_debug_scan_tmp_bytes(n), poison)
    d_owner, sp, cap = None, 0, 0
    if span is not None:
        sp, cap = span
        d_owner = _dev(np.full(cap + R.GUARD, R.SENTINEL, dtype=U32))
    _check(lib.splatraster_debug_scan_u32(n, _p(d_in), _p(d_perm), _p(d_out), _p(d_total), int(exclusive), _p(d_owner), sp, cap,
                                          _p(tmp), _stream()), "scan")
    torch.cuda.current_stream().synchronize()
    if mode == "inclusive" and n:
        assert np.array_equal(_host(d_in), values), "the input of an out-of-place scan was written"
    out = _host(d_out) if n else np.zeros(0, dtype=U32)
    return out, int(d_total.cpu().numpy().view(np.uint64)[0]), (_host(d_owner) if d_owner is not None else None), tmp


def _check_scan_case(name, mode, **kw):
    v, perm = R.scan_data(name)
    out, total, _, tmp = run_scan(v, perm, mode, **kw)
    ref, ref_total = R.scan_expected(name, mode == "exclusive in place")
    assert total == ref_total, (name, mode, total, ref_total)
    bad = np.flatnonzero(out != ref)
    assert not len(bad), (name, mode, f"{len(bad)} words differ, the first at {bad[:4].tolist()}")
    return tmp


@pytest.mark.parametrize("name", list(R.scan_cases()))
def test_scan_matches_cumsum(name):
    c = R.scan_cases()[name]
    assert _lib().splatraster_debug_scan_path(c["n"]) == c["path"]
    for mode in c["modes"]:
        _check_scan_case(name, mode)


@pytest.mark.parametrize("name", ["n 2049", "n 131073", "perm, n 2049", "n 4194305"])
def test_scan_twice_on_the_same_tmp(name):
    """the second call finds the first one's tickets and status words in tmp, and clears them itself"""
    mode = R.scan_cases()[name]["modes"][0]
    tmp = _check_scan_case(name, mode)
    _check_scan_case(name, mode, tmp=tmp)
    _check_scan_case(name, "inclusive" if R.scan_cases()[name]["perm"] else "exclusive in place", tmp=tmp)


@pytest.mark.parametrize("name", list(R.span_cases()))
def test_span_owners(name):
    c = R.span_cases()[name]
    assert _lib().splatraster_debug_scan_path(c["n"]) == c["path"]
    v = R.span_data(name)
    ref, ref_total = R.scan_ref(v)
    out, total, owner, _ = run_scan(v, None, "inclusive", span=(R.SPAN, c["cap"]))
    assert total == ref_total and np.array_equal(out, ref)
    if c["path"] == 1:
        want = R.span_owner_ref(np.cumsum(v, dtype=np.uint64), R.SPAN, c["cap"], size=c["cap"] + R.GUARD)
    else:
        want = np.full(c["cap"] + R.GUARD, R.SENTINEL, dtype=U32)      # the three-kernel form writes none (binning.hip relies on it)
    bad = np.flatnonzero(owner != want)
    assert not len(bad), (name, f"{len(bad)} entries differ, the first at {bad[:4].tolist()}: {owner[bad[:4]]} != {want[bad[:4]]}")


# ---- sort ----------------------------------------------------------------------------------------------------------------------
def run_sort(keys, vals, key_bits, keys16=False, poison=True):
    """one call of the sort (or of its uint16_t form) on the current stream: (keys, vals) as host arrays"""
    lib = _lib()
    n = len(keys)
    if keys16:
        buf = np.zeros(n, dtype=U32)
        buf.view(np.uint16)[:n] = keys.astype(np.uint16)
        buf.view(np.uint16)[n:] = 0xFFFF                      # the second half is scratch: its contents must not matter
        d_k = _dev(buf)
    else:
        d_k = _dev(keys) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_v = _dev(vals) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    tmp = _tmp(lib.splatraster_sort_tmp_bytes(n), poison)
    fn = lib.splatraster_debug_sort_pairs_k16 if keys16 else lib.splatraster_sort_pairs_u32
    _check(fn(n, _p(d_k), _p(d_v), key_bits, _p(tmp), _stream()), "sort")
    torch.cuda.current_stream().synchronize()
    return _host(d_k)[:n], _host(d_v)[:n]


def _check_sort_case(n, kb, kset, keys16=False):
    c = R.sort_case(n, kb, kset, keys16)
    assert _lib().splatraster_debug_sort_path(n, kb, int(keys16)) == c["path"], c["name"]
    keys, vals, rk, rv = R.sort_data(n, kb, kset)
    gk, gv = run_sort(keys, vals, kb, keys16)
    bad = np.flatnonzero((gk != rk) | (gv != rv))
    assert not len(bad), (c["name"], f"{len(bad)} pairs differ, the first at {bad[:4].tolist()}")
    return gk, gv


@pytest.mark.parametrize("n", R.SORT_NS)
@pytest.mark.parametrize("key_bits", R.KEY_BITS)
def test_sort_is_stable_and_exact_at_every_key_set(n, key_bits):
    for kset in R.sort_sets(n, key_bits):
        _check_sort_case(n, key_bits, kset)


def test_sort_of_nothing_leaves_the_arrays():
    for (n, kb, kset, k16) in R.sort_case_names()[:2]:
        assert _lib().splatraster_debug_sort_path(n, kb, 0) == 0
        if n:
            _check_sort_case(n, kb, kset)
        else:
            run_sort(np.zeros(0, dtype=U32), np.zeros(0, dtype=U32), kb)


@pytest.mark.parametrize("n", R.K16_NS)
@pytest.mark.parametrize("key_bits", R.K16_BITS)
def test_sort_k16_equals_the_u32_sort_and_the_reference(n, key_bits):
    for kset in R.K16_SETS:
        gk, gv = _check_sort_case(n, key_bits, kset, keys16=True)
        keys, vals, _, _ = R.sort_data(n, key_bits, kset)
        assert _lib().splatraster_debug_sort_path(n, key_bits, 0) == 3
        wk, wv = run_sort(keys, vals, key_bits)                 # the same keys, widened
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (n, key_bits, kset)


def _random_words(n, gen):
    """n random full 32-bit words as int32, made on the device"""
    hi = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int32, device=DEV, generator=gen)
    hi <<= 16
    hi |= torch.randint(0, 1 << 16, (n,), dtype=torch.int32, device=DEV, generator=gen)
    return hi


@pytest.mark.parametrize("case", R.BIG_SORTS, ids=lambda c: c["name"])
def test_sort_whose_table_scan_takes_three_kernels(case):
    """16385 blocks, one key in the last: the [256][16385] table is 2049 scan tiles, one more than the one-pass look-back takes.
    Keys, values and the reference (torch.sort, stable) stay on the device: about 3 GB."""
    lib = _lib()
    n, kb, k16 = case["n"], case["key_bits"], case["keys16"]
    assert lib.splatraster_debug_sort_path(n, kb, int(k16)) == case["path"]
    assert lib.splatraster_debug_scan_path(-(-n // 4096) * 256) == 2
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n + kb)
    keys = torch.randint(0, 1 << kb, (n,), dtype=torch.int32, device=DEV, generator=gen)
    vals = _random_words(n, gen)
    rk, order = torch.sort(keys, stable=True)
    rv = vals[order]
    del order
    if k16:
        d_k = torch.empty(n, dtype=torch.int32, device=DEV)
        d_k.view(torch.int16)[:n] = ((keys + 32768) % 65536 - 32768).to(torch.int16)       # 0 .. 65535 as their low 16 bits
        d_k.view(torch.int16)[n:] = -1
    else:
        d_k = keys.clone()
    del keys
    tmp = torch.empty(lib.splatraster_sort_tmp_bytes(n), dtype=torch.uint8, device=DEV)
    fn = lib.splatraster_debug_sort_pairs_k16 if k16 else lib.splatraster_sort_pairs_u32
    _check(fn(n, _p(d_k), _p(vals), kb, _p(tmp), _stream()), "sort")
    torch.cuda.synchronize()
    same_k, same_v = torch.equal(d_k, rk), torch.equal(vals, rv)
    ties = int((rk[1:] == rk[:-1]).sum())
    del d_k, vals, rk, rv, tmp
    torch.cuda.empty_cache()
    assert same_k and same_v and ties > n // 2


# ---- another stream, poisoned tmp ----------------------------------------------------------------------------------------------------
def test_side_stream_and_poisoned_tmp():
    """three scan and three sort cases on a stream of their own; every tmp starts as 0xFF bytes (run_scan / run_sort poison
    it): each entry point clears the state it needs"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        _check_scan_case("n 266245", "inclusive")
        _check_scan_case("perm, n 131073", "inclusive")
        _check_scan_case("n 4194305", "exclusive in place")
        _check_sort_case(4097, 32, "float32 depths")
        _check_sort_case(524_289, 17, "uniform")
        _check_sort_case(1_048_577, 16, "uniform", keys16=True)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
