"""CPU side of the scan / radix-sort edge tests (tests/test_host_scan_sort_edges.py, tests/test_gpu_scan_sort_edges.py): the
references (np.cumsum, a stable argsort), deliberately wrong models of both, and one builder per named case.  Everything is integer
arithmetic and every comparison is bit for bit.  Every case is made from a seed (the CRC of its name) or by construction; nothing
is read from disk.  Builders are cached: the arrays of the large sizes and their references are shared by the tests that use them
and must not be written to.

A case is a dict: `name`, `n`, `path` (what splatraster_debug_scan_path / _sort_path must answer for it) and `catches`, the wrong
models that must differ from the reference on the case's data (the host test checks this, so the device test cannot pass
vacuously).  Sizes mirror splatloc_amd/csrc/scan_sort.hip: a scan tile is 2048 words, at most 2048 tiles go through the one-pass
look-back; a sort block is 4096 keys (2048 in the small one-sweep form).
"""
import functools
import zlib

import numpy as np

SENTINEL = 0xDEADBEEF     # pre-fill of a span_owner buffer
GUARD = 64                # entries behind `cap` that nobody may write
SCAN_TILE = 2048
SCAN_ONEPASS_MAX = SCAN_TILE * 2048          # the last size of the one-pass scan
SORT_BIG_N = 16385 * 4096 - 4095             # 16385 blocks, one key in the last: a table of 2049 scan tiles
U32 = np.uint32


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- references --------------------------------------------------------------------------------------------------------------
def scan_ref(values, perm=None, exclusive=False):
    """(out, total): out[i] = sum of v[0..i] (v[0..i) when exclusive) mod 2^32 as uint32, total the exact sum as a Python int;
    v = values, or values[perm & 0xFFFFFF] with a packed permutation"""
    v = np.asarray(values, dtype=np.uint64)
    if perm is not None:
        v = v[np.asarray(perm, dtype=np.uint64) & np.uint64(0xFFFFFF)]
    incl = np.cumsum(v, dtype=np.uint64)
    total = int(incl[-1]) if len(v) else 0
    out = incl - v if exclusive else incl
    return (out & np.uint64(0xFFFFFFFF)).astype(U32), total


def pack_perm(values, rows):
    """the rasterizer's packed depth order (preprocess): row | min(values[row], 255) << 24"""
    rows = np.asarray(rows, dtype=U32)
    assert len(values) <= 1 << 24 and (rows < len(values)).all()
    return rows | (np.minimum(np.asarray(values, dtype=U32)[rows], U32(255)) << U32(24))


def span_owner_ref(incl, span, cap, sentinel=SENTINEL, size=None):
    """[size or cap] uint32: entry b < cap with b * span < total holds the unique i with excl[i] <= b * span < incl[i]; every
    other entry keeps `sentinel`.  `incl` is the exact inclusive scan (total < 2^32)."""
    incl = np.asarray(incl, dtype=np.uint64)
    total = int(incl[-1]) if len(incl) else 0
    assert total < 1 << 32
    buf = np.full(cap if size is None else size, sentinel, dtype=U32)
    nb = min(cap, -(-total // span), len(buf))
    targets = np.arange(nb, dtype=np.uint64) * np.uint64(span)
    buf[:nb] = np.searchsorted(incl, targets, side="right").astype(U32)      # the first i with incl[i] > b * span
    return buf


def sorted_bits(key_bits):
    """the sort moves whole 8-bit digits: the bits it orders by"""
    return 8 * ((key_bits + 7) // 8)


def _stable_order(k):
    if len(k) and int(k.max()) < 1 << 16:
        k = k.astype(np.uint16)          # numpy's stable sort of 16-bit keys is a radix sort
    return np.argsort(k, kind="stable")


def sort_ref(keys, vals, key_bits):
    """(keys, vals) in the stable order of keys & (2^(8 ceil(key_bits / 8)) - 1); whole keys travel, bits above the sorted digits
    included"""
    keys, vals = np.asarray(keys, dtype=U32), np.asarray(vals, dtype=U32)
    order = _stable_order(keys & U32((1 << sorted_bits(key_bits)) - 1))
    return keys[order], vals[order]


# ---- deliberately wrong models (host test only) --------------------------------------------------------------------------------------
def sort_unstable(keys, vals, key_bits):
    """ties come out in reverse input order"""
    keys, vals = np.asarray(keys, dtype=U32), np.asarray(vals, dtype=U32)
    m = keys & U32((1 << sorted_bits(key_bits)) - 1)
    order = len(m) - 1 - _stable_order(m[::-1])
    return keys[order], vals[order]


def sort_skip_digit(keys, vals, key_bits, k):
    """an LSD sort whose pass over digit k never ran"""
    keys, vals = np.asarray(keys, dtype=U32), np.asarray(vals, dtype=U32)
    m = keys & U32(((1 << sorted_bits(key_bits)) - 1) & ~(0xFF << (8 * k)))
    order = _stable_order(m)
    return keys[order], vals[order]


def sort_drop_value_high(keys, vals, key_bits):
    """values lose bits 24..31 on the way"""
    k, v = sort_ref(keys, vals, key_bits)
    return k, v & U32(0xFFFFFF)


def scan_total32(values, perm=None, exclusive=False):
    out, total = scan_ref(values, perm, exclusive)
    return out, total & 0xFFFFFFFF


def scan_never_gathers(values, perm, exclusive=False):
    """trusts the packed byte even at 255"""
    return scan_ref(np.asarray(perm, dtype=U32) >> U32(24), None, exclusive)


def span_owner_ignores_cap(incl, span, cap, sentinel=SENTINEL, size=None):
    size = cap if size is None else size
    return span_owner_ref(incl, span, size, sentinel, size)


# ---- scan cases -----------------------------------------------------------------------------------------------------------------
SCAN_NS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 2048 * 64 + 1, 2048 * 130 + 5, SCAN_ONEPASS_MAX, SCAN_ONEPASS_MAX + 1)
SCAN_MODES = ("inclusive", "inclusive in place", "exclusive in place")
SCAN_SMALL, SCAN_MULTI = 513, 2048 * 64 + 1
PERM_NS = (2049, 2048 * 64 + 1, SCAN_ONEPASS_MAX + 1)
PERM_VALUES = (0, 1, 254, 255, 256, 1000, 70_000)


def scan_path_of(n):
    return 0 if n <= 0 else (1 if n <= SCAN_ONEPASS_MAX else 2)


def _scan_case(name, n, **kw):
    return dict(name=name, n=n, path=scan_path_of(n), perm=False, modes=SCAN_MODES, catches=(), **kw)


def scan_cases():
    """every scan case but the span_owner ones, by name"""
    cases = [_scan_case("empty", 0, values_of="zero")]
    cases += [_scan_case(f"n {n}", n, values_of="0..7") for n in SCAN_NS]
    for n in (SCAN_SMALL, SCAN_MULTI):
        cases += [_scan_case(f"all zero, n {n}", n, values_of="zero"), _scan_case(f"all one, n {n}", n, values_of="one")]
    cases.append(dict(_scan_case("total past 2^32, n 8192", 8192, values_of="2^20"), catches=("total32",)))
    for n in PERM_NS:
        cases.append(dict(_scan_case(f"perm, n {n}", n, values_of="perm"), perm=True, modes=SCAN_MODES[:1], catches=("never gathers",)))
    return {c["name"]: c for c in cases}


@functools.lru_cache(maxsize=None)
def scan_data(name):
    """(values, perm or None) of a scan case; read-only"""
    c = scan_cases()[name]
    n, rng = c["n"], _rng("scan " + name)
    kind = c["values_of"]
    perm = None
    if kind == "zero":
        v = np.zeros(n, dtype=U32)
    elif kind == "one":
        v = np.ones(n, dtype=U32)
    elif kind == "0..7":
        v = rng.integers(0, 8, size=n, dtype=np.uint64).astype(U32)
    elif kind == "2^20":
        # every tile of 2048 sums to at most 2^31, the 8192 values to about 1.75 * 2^32
        v = rng.integers((1 << 20) - (1 << 18), 1 << 20, size=n, endpoint=True, dtype=np.uint64).astype(U32)
    else:
        v = np.asarray(PERM_VALUES, dtype=U32)[rng.integers(0, len(PERM_VALUES), size=n)]
        perm = pack_perm(v, rng.permutation(n))
        perm.setflags(write=False)
    v.setflags(write=False)
    return v, perm


@functools.lru_cache(maxsize=None)
def scan_expected(name, exclusive):
    v, perm = scan_data(name)
    out, total = scan_ref(v, perm, exclusive)
    out.setflags(write=False)
    return out, total


SPAN, SPAN_CAP = 1024, 1 << 16       # EMIT_SPAN, SPAN_OWNER_CAP: what the rasterizer passes


def span_cases():
    return {c["name"]: c for c in (
        dict(name="span owners, cap 65536", n=6151, path=1, cap=SPAN_CAP, values_of="mixed", catches=()),
        dict(name="span owners, cap 3", n=6151, path=1, cap=3, values_of="mixed", catches=("ignores cap",)),
        dict(name="span owners, total past cap * span", n=2048 * 64 + 1, path=1, cap=SPAN_CAP, values_of="0..2047",
             catches=("ignores cap",)),
        dict(name="span owners, three kernels", n=SCAN_ONEPASS_MAX + 1, path=2, cap=SPAN_CAP, values_of="0..7", catches=()),
    )}


@functools.lru_cache(maxsize=None)
def span_data(name):
    """values of a span_owner case: elements larger than a span (they own several), exact multiples of it, runs of zeros (they
    own none)"""
    c = span_cases()[name]
    n, rng = c["n"], _rng("span " + c["values_of"] + str(c["n"]))
    if c["values_of"] == "0..7":
        v = rng.integers(0, 8, size=n, dtype=np.uint64).astype(U32)
    elif c["values_of"] == "0..2047":
        v = rng.integers(0, 2048, size=n, dtype=np.uint64).astype(U32)
        v[1000:1400] = 0
        v[2048 * 40 - 3:2048 * 40 + 300] = 0
    else:
        v = rng.integers(0, 8, size=n, dtype=np.uint64).astype(U32)
        v[0:5] = 0                                   # span 0 is owned by the first non-zero element, not by element 0
        v[300:700] = 0
        v[2040:2060] = 0                             # a run across the tile boundary
        v[100], v[701], v[2047], v[2060], v[4096], v[4097], v[6150] = 3000, 1024, 5000, 2048, 1, 1023, 4000
    v.setflags(write=False)
    return v


# ---- sort cases -----------------------------------------------------------------------------------------------------------------
SORT_SMALL_NS = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097)
SORT_BOUNDARY_NS = (524_288, 524_289, 1_048_576, 1_048_577)
SORT_NS = SORT_SMALL_NS + SORT_BOUNDARY_NS
SORT_SET_NS = (2049, 4097)                   # every key set runs at these
KEY_BITS = (1, 7, 8, 9, 16, 17, 24, 25, 32)
FIRST_SETS = ("uniform", "all equal 0", "all equal max", "ascending", "descending")
K16_NS = (1_048_577, 257 * 4096)
K16_BITS = (8, 9, 16)
K16_SETS = ("uniform", "all equal max", "i % 256")


def sort_path_of(n, key_bits, keys16=False):
    if n <= 0 or key_bits <= 0:
        return 0
    if n <= 524_288:
        return 1
    if n <= 1_048_576:
        return 2
    return (4 if keys16 else 3) + (8 if -(-n // 4096) * 256 > SCAN_ONEPASS_MAX else 0)


def _passes(key_bits):
    return (key_bits + 7) // 8


def sort_sets(n, key_bits):
    """names of the key sets that run at (n, key_bits)"""
    sets = []
    if n in SORT_BOUNDARY_NS or n in SORT_SET_NS:
        sets += FIRST_SETS
    else:
        sets.append("uniform")
    if n in SORT_SET_NS:
        sets += [f"only byte {k} varies" for k in range(_passes(key_bits))]
        sets += ["i % 64", "i % 256", "(i // 64) % 256", "99 % one key"]
        if key_bits == 32:
            sets.append("float32 depths")
        if key_bits in (16, 24):
            sets.append("random bits above the sorted digits")
    return sets


def _catches(kset, n, key_bits):
    """the wrong models a set must expose; values are random 32-bit words everywhere, so a dropped value byte always shows"""
    c = ["drops value bits 24..31"]
    lim = 1 << key_bits
    if n >= 2 and (kset.startswith("all equal") or kset == "99 % one key" or (kset.startswith("i %") and n > 256)
                   or (kset.startswith("(i //") and n > 64) or (kset == "float32 depths")):
        c.append("unstable")
    if kset == "uniform" and n >= 2049:
        c.append("unstable" if n > 4 * lim else None)
        # a skipped digit k shows on pairs that agree above it: about n^2 / 4 / 256^(digits above k) of them
        p = _passes(key_bits)
        c += [f"skips digit {k}" for k in range(p) if n * n >= 256 << (8 * (p - 1 - k))]
    if kset.startswith("only byte"):
        c.append(f"skips digit {int(kset.split()[2])}")
        c.append("unstable")
    if kset == "descending" and n >= 2:
        c.append(f"skips digit {_passes(key_bits) - 1}")          # the top digit alone already reverses the input
    if kset == "float32 depths":
        c += [f"skips digit {k}" for k in range(4)]
    if kset == "random bits above the sorted digits":
        c.append("carries no upper bits")
    return tuple(x for x in c if x)


def sort_case_names():
    """(n, key_bits, set, keys16) of every sort case but the two large ones"""
    out = [(0, 8, "uniform", False), (5, 0, "uniform", False)]       # nothing to do: the arrays stay as they are
    for n in SORT_NS:
        for kb in KEY_BITS:
            out += [(n, kb, s, False) for s in sort_sets(n, kb)]
    for n in K16_NS:
        for kb in K16_BITS:
            out += [(n, kb, s, True) for s in K16_SETS]
    return out


def sort_case(n, key_bits, kset, keys16=False):
    return dict(name=f"{'k16 ' if keys16 else ''}n {n}, {key_bits} bits, {kset}", n=n, key_bits=key_bits, set=kset, keys16=keys16,
                path=sort_path_of(n, key_bits, keys16), catches=_catches(kset, n, key_bits) if n and key_bits else ())


def float_depth_keys(n, rng):
    """bit patterns of positive float32 depths as the depth sort sees them: duplicates (depths quantised to 1/64), denormals, 0
    and +inf"""
    d = (np.round(rng.uniform(0.2, 100.0, size=n) * 64) / 64).astype(np.float32)
    k = d.view(U32).copy()
    idx = rng.permutation(n)
    q = max(1, n // 50)
    k[idx[:q]] = rng.integers(1, 1 << 23, size=q, dtype=np.uint64).astype(U32)      # denormals
    k[idx[q:2 * q]] = U32(0x7F800000)                                              # +inf
    k[idx[2 * q:3 * q]] = U32(0)
    k[idx[3 * q:4 * q]] = U32(1)                                                   # the smallest denormal, many times
    return k


@functools.lru_cache(maxsize=64)
def sort_values(n):
    """random full 32-bit words; element 0 has bit 31 set so that even n = 1 carries a high byte"""
    v = _rng(f"sort values {n}").integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U32)
    if n:
        v[0] |= U32(1 << 31)
    v.setflags(write=False)
    return v


def sort_keys(n, key_bits, kset):
    """the keys of a case (below 2^key_bits unless the set says otherwise)"""
    rng = _rng(f"sort keys {n} {key_bits} {kset}")
    lim = 1 << max(key_bits, 1)
    mask = U32(lim - 1)
    i = np.arange(n, dtype=np.uint64)
    if kset == "uniform":
        k = rng.integers(0, lim, size=n, dtype=np.uint64)
    elif kset == "all equal 0":
        k = np.zeros(n, dtype=np.uint64)
    elif kset == "all equal max":
        k = np.full(n, lim - 1, dtype=np.uint64)
    elif kset == "ascending":
        k = i * np.uint64(lim) // np.uint64(max(n, 1))                  # non-decreasing over the whole range
    elif kset == "descending":
        k = np.uint64(lim - 1) - i * np.uint64(lim) // np.uint64(max(n, 1))
    elif kset.startswith("only byte"):
        b = int(kset.split()[2])
        width = min(8, key_bits - 8 * b)
        const = 0xA5A5A5A5 & (lim - 1) & ~(0xFF << (8 * b))
        k = np.uint64(const) | (rng.integers(0, 1 << width, size=n, dtype=np.uint64) << np.uint64(8 * b))
    elif kset == "i % 64":
        k = i % np.uint64(64)
    elif kset == "i % 256":
        k = i % np.uint64(256)
    elif kset == "(i // 64) % 256":
        k = (i // np.uint64(64)) % np.uint64(256)
    elif kset == "99 % one key":
        k = np.full(n, (lim - 1) * 2 // 3, dtype=np.uint64)
        where = rng.permutation(n)[:max(1, n // 100)]
        k[where] = rng.integers(0, lim, size=len(where), dtype=np.uint64)
    elif kset == "float32 depths":
        return float_depth_keys(n, rng)
    elif kset == "random bits above the sorted digits":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U32)
    else:
        raise KeyError(kset)
    return k.astype(U32) & mask


@functools.lru_cache(maxsize=16)          # 12 MB an entry: the tests that share a large case run next to each other
def _sort_data_big(n, key_bits, kset):
    k, v = sort_keys(n, key_bits, kset), sort_values(n)
    rk, rv = sort_ref(k, v, key_bits)
    for a in (k, rk, rv):
        a.setflags(write=False)
    return k, v, rk, rv


def sort_data(n, key_bits, kset):
    """(keys, vals, sorted keys, sorted vals); read-only at the large sizes, which are cached"""
    if n >= SORT_BOUNDARY_NS[0]:
        return _sort_data_big(n, key_bits, kset)
    k, v = sort_keys(n, key_bits, kset), sort_values(n)
    return (k, v) + sort_ref(k, v, key_bits)


def wrong_sort(model, keys, vals, key_bits):
    if model == "unstable":
        return sort_unstable(keys, vals, key_bits)
    if model.startswith("skips digit"):
        return sort_skip_digit(keys, vals, key_bits, int(model.split()[2]))
    if model == "drops value bits 24..31":
        return sort_drop_value_high(keys, vals, key_bits)
    if model == "carries no upper bits":
        k, v = sort_ref(keys, vals, key_bits)
        return k & U32((1 << sorted_bits(key_bits)) - 1), v
    raise KeyError(model)


# the two sorts whose table scan takes three kernels (keys, values and reference are made on the device)
BIG_SORTS = (dict(name="three-kernel table scan", n=SORT_BIG_N, key_bits=8, keys16=False, path=3 + 8),
             dict(name="three-kernel table scan, k16", n=SORT_BIG_N, key_bits=16, keys16=True, path=4 + 8))
