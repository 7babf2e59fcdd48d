"""The oracle of tests/test_gpu_scan_sort_edges.py, pinned on the host: the references of tests/scan_sort_reference.py on
hand-worked arrays, proof that every case takes the path of the library its name claims (the host-only hooks
splatraster_debug_sort_path / _scan_path) and that together the cases reach every path, and proof that every case's data exposes
the wrong model it was built for, so that the device tests cannot pass vacuously.  No test here touches a GPU."""
import numpy as np
import pytest

from tests import scan_sort_reference as R

U32 = np.uint32


def _lib():
    from splatloc_amd import _native
    return _native.load()


# ---- the reference, by hand ---------------------------------------------------------------------------------------------------------
def test_scan_reference_by_hand():
    v = np.array([3, 0, 5, 0xFFFFFFFF, 1], dtype=U32)
    out, total = R.scan_ref(v)
    assert out.tolist() == [3, 3, 8, 7, 8] and total == (1 << 32) + 8            # 8 + 0xFFFFFFFF wraps to 7
    out, total = R.scan_ref(v, exclusive=True)
    assert out.tolist() == [0, 3, 3, 8, 7] and total == (1 << 32) + 8
    assert R.scan_total32(v)[1] == 8
    # packed permutation: rows 2, 0, 1 of (1, 300, 255); 255 and 300 both pack to 255
    vals = np.array([1, 300, 255], dtype=U32)
    perm = R.pack_perm(vals, [2, 0, 1])
    assert perm.tolist() == [(255 << 24) | 2, (1 << 24) | 0, (255 << 24) | 1]
    assert R.scan_ref(vals, perm)[0].tolist() == [255, 256, 556] and R.scan_ref(vals, perm)[1] == 556
    assert R.scan_never_gathers(vals, perm)[0].tolist() == [255, 256, 511]
    assert R.scan_ref(np.zeros(0, dtype=U32))[1] == 0
    # span owners: inclusive (0, 0, 5, 5, 12, 13), span 4: targets 0, 4, 8, 12 are owned by elements 2, 2, 4, 5
    incl = R.scan_ref(np.array([0, 0, 5, 0, 7, 1], dtype=U32))[0]
    S = R.SENTINEL
    assert R.span_owner_ref(incl, 4, 6).tolist() == [2, 2, 4, 5, S, S]
    assert R.span_owner_ref(incl, 4, 3, size=5).tolist() == [2, 2, 4, S, S]
    assert R.span_owner_ignores_cap(incl, 4, 3, size=5).tolist() == [2, 2, 4, 5, S]
    assert R.span_owner_ref(R.scan_ref(np.zeros(4, dtype=U32))[0], 4, 3).tolist() == [S, S, S]      # a total of 0 owns nothing


def test_sort_reference_by_hand():
    keys = np.array([0x0102, 0x0001, 0x0102, 0x10001, 0x0000], dtype=U32)
    vals = np.array([10, 11, 12, 0xFF000013, 14], dtype=U32)
    k, v = R.sort_ref(keys, vals, 16)
    # 0x10001 sorts as 0x0001 (bit 16 rides along), behind the 0x0001 that came first
    assert k.tolist() == [0, 1, 0x10001, 0x0102, 0x0102] and v.tolist() == [14, 11, 0xFF000013, 10, 12]
    k, v = R.sort_ref(keys, vals, 9)                               # 9 bits sort two whole digits
    assert k.tolist() == [0, 1, 0x10001, 0x0102, 0x0102]
    k, v = R.sort_ref(keys, vals, 8)                               # one digit: 0x0102 sorts as 2
    assert k.tolist() == [0, 1, 0x10001, 0x0102, 0x0102] and v.tolist() == [14, 11, 0xFF000013, 10, 12]
    k, v = R.sort_ref(keys, vals, 17)
    assert k.tolist() == [0, 1, 0x0102, 0x0102, 0x10001] and v.tolist() == [14, 11, 10, 12, 0xFF000013]
    k, v = R.sort_unstable(keys, vals, 16)
    assert v.tolist() == [14, 0xFF000013, 11, 12, 10]
    k, v = R.sort_skip_digit(keys, vals, 16, 0)                    # only digit 1 sorted: (1, 0, 1, 0, 0) keeps input order within
    assert v.tolist() == [11, 0xFF000013, 14, 10, 12]
    assert R.sort_drop_value_high(keys, vals, 16)[1].tolist() == [14, 11, 0x13, 10, 12]
    assert [R.sorted_bits(b) for b in (1, 7, 8, 9, 16, 17, 24, 25, 32)] == [8, 8, 8, 16, 16, 24, 24, 32, 32]


# ---- paths ----------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_path_it_names_and_every_path_is_taken():
    lib = _lib()
    scan_seen, sort_seen = set(), set()
    for c in list(R.scan_cases().values()) + list(R.span_cases().values()):
        assert lib.splatraster_debug_scan_path(c["n"]) == c["path"] == R.scan_path_of(c["n"]), c["name"]
        scan_seen.add(c["path"])
    cases = [R.sort_case(*a) for a in R.sort_case_names()] + list(R.BIG_SORTS)
    for c in cases:
        assert lib.splatraster_debug_sort_path(c["n"], c["key_bits"], int(c["keys16"])) == c["path"], c["name"]
        sort_seen.add(c["path"])
        # a table scan inside a sort takes the three-kernel form exactly when the case says + 8
        if c["path"] >= 3:
            words = -(-c["n"] // 4096) * 256
            assert (lib.splatraster_debug_scan_path(words) == 2) == bool(c["path"] & 8), c["name"]
    assert scan_seen == {0, 1, 2}
    assert sort_seen == {0, 1, 2, 3, 4, 3 + 8, 4 + 8}
    # everything the hooks can answer besides: the refusal
    assert lib.splatraster_debug_scan_path(-1) == -1
    for bad in ((-1, 8, 0), (5, -1, 0), (5, 33, 0), (1_048_576, 8, 1), (1_048_577, 17, 1), (0, 8, 1)):
        assert lib.splatraster_debug_sort_path(*bad) == -1, bad
    print(f"{len(cases)} sort cases over paths {sorted(sort_seen)}, "
          f"{len(R.scan_cases()) + len(R.span_cases())} scan cases over paths {sorted(scan_seen)}")


def test_path_boundaries_sit_where_the_cases_put_them():
    lib = _lib()
    sp, cp = lib.splatraster_debug_sort_path, lib.splatraster_debug_scan_path
    assert [sp(n, 32, 0) for n in R.SORT_BOUNDARY_NS] == [1, 2, 2, 3]
    assert [sp(n, 16, 0) for n in (1, 4097)] == [1, 1]
    assert [sp(n, 8, 0) for n in (R.SORT_BIG_N - 1, R.SORT_BIG_N)] == [3, 11]
    assert [sp(n, 16, 1) for n in R.K16_NS + (R.SORT_BIG_N - 1, R.SORT_BIG_N)] == [4, 4, 4, 12]
    assert [cp(n) for n in (R.SCAN_ONEPASS_MAX, R.SCAN_ONEPASS_MAX + 1)] == [1, 2]
    # the three-kernel scan of 2048 * 2048 + 1 words reduces 2049 partials: rounds of 1024 + 1024 + 1
    assert -(-(R.SCAN_ONEPASS_MAX + 1) // R.SCAN_TILE) == 2049
    assert -(-(-(-R.SORT_BIG_N // 4096) * 256) // R.SCAN_TILE) == 2049 and R.SORT_BIG_N % 4096 == 1
    assert lib.splatraster_debug_scan_tmp_bytes(R.SCAN_ONEPASS_MAX + 1) >= 8 * (2049 + 2)
    assert lib.splatraster_debug_scan_tmp_bytes(0) > 0


def test_case_lists_hold_what_the_issue_lists():
    names = R.sort_case_names()
    for n in R.SORT_NS:
        for kb in R.KEY_BITS:
            assert (n, kb, "uniform", False) in names
    for n in R.SORT_BOUNDARY_NS + R.SORT_SET_NS:
        for kb in R.KEY_BITS:
            assert all((n, kb, s, False) in names for s in R.FIRST_SETS)
    for n in R.SORT_SET_NS:
        for kb in R.KEY_BITS:
            sets = R.sort_sets(n, kb)
            assert [s for s in sets if s.startswith("only byte")] == [f"only byte {k} varies" for k in range((kb + 7) // 8)]
            assert {"i % 64", "i % 256", "(i // 64) % 256", "99 % one key"} <= set(sets)
            assert ("float32 depths" in sets) == (kb == 32)
            assert ("random bits above the sorted digits" in sets) == (kb in (16, 24))
    assert sum(1 for a in names if a[3]) == len(R.K16_NS) * len(R.K16_BITS) * len(R.K16_SETS)
    sc = R.scan_cases()
    assert all(f"n {n}" in sc for n in R.SCAN_NS) and all(f"perm, n {n}" in sc for n in R.PERM_NS)
    assert all(c["modes"] == R.SCAN_MODES for c in sc.values() if not c["perm"])


# ---- edges: every case's data exposes the wrong model it is there for -----------------------------------------------------------------------
def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", R.SORT_NS + R.K16_NS[1:])
def test_sort_cases_expose_their_wrong_models(n):
    caught = {}
    for (cn, kb, kset, k16) in R.sort_case_names():
        if cn != n:
            continue
        c = R.sort_case(cn, kb, kset, k16)
        keys, vals, rk, rv = R.sort_data(cn, kb, kset)
        assert len(keys) == len(vals) == n and keys.dtype == vals.dtype == U32
        if kset != "random bits above the sorted digits" and kset != "float32 depths":
            assert int(keys.max()) < 1 << kb, c["name"]
        if k16:
            assert int(keys.max()) < 1 << 16
        assert (vals >> U32(24)).any(), c["name"]                                   # value bits 24..31 are populated
        assert "drops value bits 24..31" in c["catches"]
        for model in c["catches"]:
            assert _differs(R.wrong_sort(model, keys, vals, kb), (rk, rv)), (c["name"], model)
            caught[model] = caught.get(model, 0) + 1
        if "unstable" in c["catches"]:                                              # ties carry distinct values
            m = rk & U32((1 << R.sorted_bits(kb)) - 1)
            tie = np.flatnonzero(m[1:] == m[:-1])
            assert len(tie) and (rv[tie] != rv[tie + 1]).any(), c["name"]
        if kset.startswith("only byte"):                                            # byte k really varies, and only it
            b = int(kset.split()[2])
            assert len(np.unique((keys >> U32(8 * b)) & U32(0xFF))) > 1 and len(np.unique(keys & ~U32(0xFF << (8 * b)))) == 1
        if kset == "random bits above the sorted digits":
            assert (keys >> U32(kb)).any() and len(np.unique(keys >> U32(kb))) > 100
        if kset == "float32 depths":
            f = keys.view(np.float32)
            assert np.isposinf(f).any() and ((f > 0) & (f < np.finfo(np.float32).tiny)).any() and (f == 0).any()
            assert not np.signbit(f).any() and not np.isnan(f).any() and len(np.unique(keys)) < n
            assert np.array_equal(rk.view(np.float32), np.sort(f, kind="stable"))   # positive floats sort as their bits
        if kset == "i % 64" and kb >= 8:
            assert np.array_equal(keys[:64], np.arange(64, dtype=U32))              # every lane of a wave a different digit
        if kset == "(i // 64) % 256" and kb >= 8:
            assert (keys[:64] == 0).all() and (keys[64:128] == 1).all()             # every lane of a wave the same digit
        if kset == "99 % one key":
            assert np.unique(keys, return_counts=True)[1].max() >= n * 98 // 100
    print(f"n {n}: wrong models caught: {caught}")
    assert caught
    if n >= 2049:
        assert "unstable" in caught and "skips digit 0" in caught
    if n in R.SORT_SET_NS or n in R.SORT_BOUNDARY_NS:
        assert all(f"skips digit {k}" in caught for k in range(4))


def test_scan_cases_expose_their_wrong_models():
    for name, c in R.scan_cases().items():
        v, perm = R.scan_data(name)
        assert len(v) == c["n"] and (perm is None) == (not c["perm"])
        out, total = R.scan_expected(name, False)
        if c["values_of"] not in ("zero",):
            assert total > 0 or c["n"] == 0
        if "total32" in c["catches"]:
            assert R.scan_total32(v)[1] != total and total > 1 << 32
            tiles = v.astype(np.uint64).reshape(-1, R.SCAN_TILE).sum(axis=1)       # ... while no tile does
            assert tiles.max() < 1 << 32 and c["n"] % R.SCAN_TILE == 0
            assert len(np.unique(out)) == c["n"]
        if "never gathers" in c["catches"]:
            assert (v >= 255).any() and (v < 255).any() and set(np.unique(v).tolist()) == set(R.PERM_VALUES)
            rows = perm & U32(0xFFFFFF)
            assert np.array_equal(np.sort(rows), np.arange(c["n"], dtype=U32)) and not np.array_equal(rows, np.arange(c["n"]))
            assert np.array_equal(perm >> U32(24), np.minimum(v[rows], 255))
            assert _differs(R.scan_never_gathers(v, perm), (out, total))
        if c["values_of"] == "0..7":
            assert set(np.unique(v).tolist()) <= set(range(8)) and (c["n"] < 64 or len(np.unique(v)) == 8)
    # the exclusive form of a case is not its inclusive form
    assert _differs(R.scan_expected("n 9", True), R.scan_expected("n 9", False))


def test_span_cases_expose_their_wrong_models():
    for name, c in R.span_cases().items():
        v = R.span_data(name)
        incl, total = R.scan_ref(v)
        assert total < 1 << 32 and int(incl[-1]) == total
        cap, size = c["cap"], c["cap"] + R.GUARD
        ref = R.span_owner_ref(incl.astype(np.uint64), R.SPAN, cap, size=size)
        assert (ref[cap:] == R.SENTINEL).all()
        owners = ref[ref != R.SENTINEL]
        if "ignores cap" in c["catches"]:                                           # cap really truncates
            assert total > cap * R.SPAN and len(owners) == cap
            assert _differs([R.span_owner_ignores_cap(incl.astype(np.uint64), R.SPAN, cap, size=size)], [ref])
        elif c["path"] == 1:
            assert len(owners) == -(-total // R.SPAN) < cap
        if c["values_of"] == "mixed":
            assert (v > R.SPAN).any() and (v == R.SPAN).any() and (v[:5] == 0).all()
            if cap > 3:
                counts = np.bincount(owners)
                assert counts.max() >= 4 and (counts[v[:len(counts)] == 0] == 0).all()   # several spans per owner; zeros own none
                assert owners[0] == 5 and (v[owners] > 0).all()
        print(f"{name}: total {total}, {len(owners)} owned spans of {cap}")
