"""The oracle of tests/test_gpu_selection_edges.py, pinned on the host: hand-computed expectations for the threshold cases, proof
that every case builder of tests/selection_reference.py reaches the edge it was built for (so the device tests cannot pass
vacuously), the rounding-sensitive pairs, and the bars: a numpy emulation of the kernel's own operation sequence stays inside
each of them.  Each test prints, per case, the edge reached and the largest err / bar ratio (pytest -s shows them)."""
import numpy as np
import pytest

from tests import selection_reference as R
from tests.test_host_selection import greedy_pick, priority_order, scores_f64


def _scores(s, **kw):
    return scores_f64(s["points"], s["w2cs"], s["K"], s["depths"], s["width"], s["height"], **kw)


def _ref(s):
    return R.reference_and_bars(s["points"], s["w2cs"], s["K"], s["depths"], s["width"], s["height"])


def _emulated(ref):
    """the kernel's own sequence in numpy, shaped like the device's result"""
    ks = ref["ks"]
    seen = ks["n_visible"] > 0
    span = np.zeros(len(seen))
    if seen.any():
        span[seen] = R.span_kernel(ks["H"][seen])[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(ks["var"])
        score = R.min2(0.05 / ks["mean"]) + R.min2(0.05 / sd) + span
    return dict(n_visible=ks["n_visible"], n_depth=ks["n_depth"], depth_mean=ks["mean"], depth_std=sd, span=span, score=score)


def _inside_bars(s, what):
    ref = _ref(s)
    worst = R.check_device_scores(_emulated(ref), ref, what)
    print(f"{what}: worst err / bar {worst}")
    return ref, worst


# ---- thresholds ---------------------------------------------------------------------------------------------------------------
def test_threshold_expectations_by_hand():
    scene, rows = R.threshold_case()
    got = _scores(scene)
    for i, (name, nv, nd, mean) in enumerate(rows):
        assert (got["n_visible"][i], got["n_depth"][i]) == (nv, nd), name
        if mean is None:
            assert nd == 0 and np.isnan(got["depth_mean"][i]), name
        else:
            assert got["depth_mean"][i] == mean and got["depth_std"][i] == 0.0, name
        print(f"threshold: {name}: n_visible {nv}, n_depth {nd}, depth_mean {mean}")
    # the kept diffs name distinct pixels
    means = [r[3] for r in rows if r[3] is not None]
    assert len(set(means)) == len(means)
    ref, _ = _inside_bars(scene, "thresholds")
    assert np.array_equal(ref["n_visible"], got["n_visible"]) and np.array_equal(ref["n_depth"], got["n_depth"])


def test_permuted_poses_see_some_points():
    s = R.permuted_threshold_case()
    got = _scores(s)
    per_view = [scores_f64(s["points"], s["w2cs"][v:v + 1], s["K"], s["depths"][v:v + 1], s["width"], s["height"])["n_visible"]
                for v in range(3)]
    assert all(0 < p.sum() < len(p) for p in per_view)
    assert np.array_equal(got["n_visible"], sum(per_view))
    _inside_bars(s, "permuted poses")


# ---- the emulation and the lookup variant agree with the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("M", R.GRID_M)
def test_grid_cases_reach_both_outcomes_and_stay_inside_the_bars(M):
    for N in R.GRID_N:
        s = R.grid_case(N, M)
        ref, worst = _inside_bars(s, f"grid N={N} M={M}")
        if M == 0:
            assert not ref["n_visible"].any()
            continue
        got = _scores(s)
        assert np.array_equal(ref["n_visible"], got["n_visible"]) and np.array_equal(ref["n_depth"], got["n_depth"])
        pairs, seen, kept = N * M, ref["n_visible"].sum(), ref["n_depth"].sum()
        if pairs >= 63:
            assert 0 < seen < pairs and 0 < kept < seen, (N, M, seen, kept)
        print(f"grid N={N} M={M}: {seen} of {pairs} pairs visible, {kept} kept")


def test_lookup_restatement_is_bit_identical_on_a_dense_case():
    s = R.grid_case(257, 65)
    dense = _scores(s)
    looked = R.scores_f64_lookup(s["points"], s["w2cs"], s["K"], lambda v, r, c: s["depths"][v, r, c], s["width"], s["height"])
    assert dense["n_depth"].sum() > 100
    for k in dense:
        assert np.array_equal(dense[k].view(np.int64 if dense[k].dtype == np.float64 else dense[k].dtype),
                              looked[k].view(np.int64 if looked[k].dtype == np.float64 else looked[k].dtype)), k


def test_big_case_marks_are_what_the_points_read():
    pts, w2cs, K, marks = R.big_case()
    M, H, W = R.BIG["M"], R.BIG["H"], R.BIG["W"]
    assert M * H * W > 2 ** 31 and (M - 1) * H * W >= 2 ** 31
    got = R.scores_f64_lookup(pts, w2cs, K, R.big_lookup(marks), W, H)
    per_point = np.zeros(len(pts), int)
    for v in (0, M - 1):
        one = R.scores_f64_lookup(pts, w2cs[v:v + 1], K, lambda _, r, c, v=v: R.big_lookup(marks)(np.full(r.shape, v), r, c), W, H)
        per_point += one["n_depth"]
        assert one["n_depth"].sum() == sum(1 for m in marks if m[0] == v) > 0       # every mark is read, in its view
    assert np.array_equal(got["n_depth"], per_point) and got["n_depth"].max() == 2 and got["n_depth"].min() == 1
    assert got["n_visible"].min() < M and got["n_visible"].max() == M
    offs = [v * H * W + r * W + c for v, r, c in marks]
    assert max(offs) == M * H * W - 1 and min(offs) == 0 and sum(o >= 2 ** 31 for o in offs) >= 5
    # an offset truncated to 31 bits lands on an unmarked pixel
    assert not any((o & 0x7fffffff) in offs for o in offs if o >= 2 ** 31)
    assert any(r >= H - 2 for _, r, _ in marks)
    print(f"big stack: {len(marks)} marks, offsets {min(offs)} .. {max(offs)}")


def test_general_k_cases_have_q2_at_and_below_zero():
    for K, exact in ((R.GENERAL_K, False), (R.ZERO_ROW_K, True)):
        s = R.general_k_case(K)
        q2 = R.q2_view0(s)
        assert (q2[-4:-1] < 0).all() if not exact else q2[-1] == 0.0
        assert (q2 <= 0).sum() >= (1 if exact else 3)
        ref, _ = _inside_bars(s, f"K third row {K[2]}")
        got = _scores(s)
        assert np.array_equal(ref["n_visible"], got["n_visible"]) and np.array_equal(ref["n_depth"], got["n_depth"])
        assert 0 < got["n_visible"].sum() < got["n_visible"].size * 9


def test_image_shape_cases_see_points():
    for w, h in R.IMAGE_SHAPES:
        s = R.image_case(w, h)
        ref, _ = _inside_bars(s, f"{w} x {h}")
        assert ref["n_visible"].sum() > 0, (w, h)
        print(f"{w} x {h}: {ref['n_visible'].sum()} visible pairs, {ref['n_depth'].sum()} kept")
    s = R.crop_case()
    ref, _ = _inside_bars(dict(s, depths=s["depths"][:, :30, :40]), "crop")
    # the poison would be kept wherever it were read: reading the stack with the window's pitch changes n_depth
    wrong = s["depths"].reshape(len(s["depths"]), -1)[:, :30 * 40].reshape(-1, 30, 40)
    bad = scores_f64(s["points"], s["w2cs"], s["K"], wrong, 40, 30)
    assert not np.array_equal(bad["n_depth"], ref["n_depth"])


# ---- Jacobi and statistics --------------------------------------------------------------------------------------------------------
def test_jacobi_cases_reach_their_matrices():
    if not R.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa here: no span bars")
    worst = 0.0
    for name, s in R.jacobi_cases().items():
        ref, w = _inside_bars(s, f"jacobi {name}")
        H = ref["ks"]["H"][0]
        off = np.abs(H[np.triu_indices(3, 1)])
        ev = np.linalg.eigvalsh(H)
        if name == "diagonal":
            assert off.max() == 0.0 and len(set(np.diag(H))) > 1
        elif name == "isotropic":
            assert off.max() == 0.0 and len(set(np.diag(H))) == 1 and ref["c"][0] == 0.0 and ref["span"][0] == np.pi / 2
        elif name == "rank-1 complement":
            assert ref["n_visible"][0] >= 2 and abs(ev[0]) < 1e-15 and off.min() > 0.1 and abs(ref["c"][0] - 1) <= R.SPAN_C_BAR
        elif name == "single off-diagonal":
            assert H[0, 1] != 0.0 and H[0, 2] == 0.0 and H[1, 2] == 0.0
        elif name == "two nearly equal":
            assert 0 < ev[2] - ev[1] < 1e-7 < ev[1] - ev[0]
        # the f64 restatement stays within a quarter of the bar
        rest = _scores(s)
        err = abs(np.cos(rest["span"][0]) - ref["c"][0])
        assert err <= R.SPAN_C_BAR / 4, (name, err)
        worst = max(worst, w["c"])
        print(f"jacobi {name}: H = {H.tolist()}, c = {ref['c'][0]!r}, restatement off by {err:.3g}")
    assert R.measure_span_c_bar() == R.SPAN_C_MEASURED          # the recorded constant is what this machine measures
    print(f"jacobi: worst kernel-sequence err / bar {worst}")


def test_statistics_cases_reach_their_edges():
    for name, (s, prop) in R.statistics_cases().items():
        ref, worst = _inside_bars(s, f"statistics {name}")
        d = ref["ks"]["diffs"][0]
        d = d[~np.isnan(d)]
        if prop == "equal":
            assert len(set(d.tolist())) == 1 and ref["var"][0] == 0.0 and ref["mean"][0] == d[0]
            assert ref["mean_bar"][0] == 0.0 and ref["var_bar"][0] == 0.0
            em = _emulated(ref)
            assert em["depth_std"][0] == 0.0 and em["depth_mean"][0] == d[0] and em["score"][0] == 0.05 / d[0] + 2.0 + em["span"][0]
        else:
            assert ref["n_depth"][0] == len(d) == prop
        if name == "one ulp apart":
            assert sorted(set(d.tolist())) == [0.125, np.nextafter(0.125, 1)]
        if name == "1 kept of 129":
            assert ref["n_visible"][0] == 129
        if name.startswith("0.2999"):
            assert 0.2998 < d.min() and d.max() < 0.3 and 5e-10 < d.max() - d.min() < 1.1e-9 and len(set(d.tolist())) > 4
            # the unshifted one-pass variance loses everything here; the shifted one is inside the bar
            naive = (d * d).sum() / len(d) - (d.sum() / len(d)) ** 2
            assert abs(naive - ref["var"][0]) > ref["var_bar"][0]
        print(f"statistics {name}: n_depth {len(d)}, mean {ref['mean'][0]!r}, var {ref['var'][0]!r}, bars "
              f"{ref['mean_bar'][0]:.3g} / {ref['var_bar'][0]:.3g}")


def test_stats_exact_is_exact():
    assert R.stats_exact([0.5, 0.25, 0.75]) == (0.5, 1.0 / 24.0)
    big = [1.0 + k * 2.0 ** -52 for k in range(3)]
    assert R.stats_exact(big) == (1.0 + 2.0 ** -52, float(R.Fraction(2, 3) * R.Fraction(2) ** -104))


# ---- order ------------------------------------------------------------------------------------------------------------------
def test_special_scores_cover_the_pool_and_order_as_documented():
    s = R.special_scores()
    bits = s.view(np.uint64)
    assert np.isnan(s).sum() > 100 and len(set(bits[np.isnan(s)].tolist())) >= 6
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    assert (s == 5e-324).any() and (s == -5e-324).any() and np.isposinf(s).any() and np.isneginf(s).any()
    hi, lo = bits >> np.uint64(32), bits & np.uint64(0xffffffff)
    fin = ~np.isnan(s)
    assert len(set(lo[fin & (hi == 0x40000000)].tolist())) >= 3 and len(set(hi[fin & (lo == 1)].tolist())) >= 4
    order = priority_order(s)
    nn = np.isnan(s).sum()
    assert np.isnan(s[order[:nn]]).all() and np.array_equal(order[:nn], np.flatnonzero(np.isnan(s))[::-1])
    assert np.isposinf(s[order[nn]]) and np.isneginf(s[order[-1]])
    z = np.flatnonzero(s[order] == 0)
    assert np.array_equal(order[z], np.flatnonzero(s == 0)[::-1])               # -0.0 ties with +0.0: the larger index first
    rest = s[order[nn:]]
    assert np.all(rest[:-1] >= rest[1:])
    # on the lattice at radius 0.25 the pick is the order
    pts = R.lattice_points(200)
    idx, trace = R.greedy_trace(pts, s[:200], 200, 0.25)
    assert np.array_equal(idx, priority_order(s[:200])) and len(trace) == 1
    for N in R.SORT_SIZES[:1]:
        t = R.tied_scores(N)
        assert len(np.unique(t)) > 60 and np.bincount(t[t == np.floor(t)].astype(int)).min() > N // 100


# ---- pick -------------------------------------------------------------------------------------------------------------------
def _passes(trace):
    return [(t["start"], t["survivors"], t["end"]) for t in trace]


def test_traced_loop_is_the_reference_loop():
    for name in ("filter 257", "chunk near 1025", "lattice under r", "rounding pair 1", "duplicates", "long pass count",
                 "many landmarks, num 4097"):
        c, idx, trace = R.traced(name)
        assert np.array_equal(idx, greedy_pick(c["points"], c["scores"], c["num"], c["radius"])), name
        assert trace[-1]["end"] == c["num"] and all(a["end"] == b["start"] for a, b in zip(trace, trace[1:]))


@pytest.mark.parametrize("num", [5000, 4096, 4097, 4098])
def test_many_landmarks_case_needs_the_global_branch(num):
    c, idx, trace = R.traced(f"many landmarks, num {num}")
    assert _passes(trace) == [(1, len(c["points"]) - 2, num)]
    pk = trace[0]["pass_killer"]
    late = (pk >= 4096).sum()
    assert late > (20 if num == 5000 else -1)
    print(f"many landmarks, num {num}: {num - 1} taken within pass 1, {late} candidates rejected only by in-pass landmark "
          f">= 4096 (largest {pk.max()})")


@pytest.mark.parametrize("S", R.CHUNK_SURVIVORS)
def test_chunk_cases_have_the_survivor_counts(S):
    c, idx, trace = R.traced(f"chunk far {S}")
    assert _passes(trace) == [(1, S, S + 1)] and (trace[0]["pass_killer"][1:] == -1).all()
    c, idx, trace = R.traced(f"chunk near {S}")
    nch = -(-S // 1024)
    assert _passes(trace)[0] == (1, S, 1 + nch) and len(trace) == 3 and trace[1]["survivors"] == 0
    pk = trace[0]["pass_killer"][trace[0]["surv"]]
    # each chunk: its first survivor is taken, every other one is killed by exactly that landmark
    for ch in range(nch):
        part = pk[ch * 1024:(ch + 1) * 1024]
        assert part[0] == -1 and (part[1:] == ch).all()
    print(f"chunk: survivors of pass 1 == {S}; far: all taken; near: {nch} taken, one per chunk")


def test_num_is_reached_inside_and_at_the_start_of_a_chunk():
    c, idx, trace = R.traced("num at first of chunk 2")
    pk = trace[0]["pass_killer"][trace[0]["surv"]]
    assert _passes(trace) == [(1, 2049, 1026)] and (pk[:1025] == -1).all() and (pk[1025:] == -2).all()
    c, idx, trace = R.traced("num inside chunk 1")
    pk = trace[0]["pass_killer"][trace[0]["surv"]]
    assert _passes(trace) == [(1, 1023, 501)] and (pk[:500] == -1).all() and (pk[500:] == -2).all() and len(pk) - 500 > 500
    print("num reached at the first candidate of chunk 2, and with 523 live candidates left in chunk 1")


@pytest.mark.parametrize("L", R.FILTER_COUNTS)
def test_filter_cases_start_a_pass_at_the_count(L):
    c, idx, trace = R.traced(f"filter {L}")
    assert len(trace) == 2 and trace[1]["start"] == L and trace[1]["end"] == c["num"] < L + trace[1]["survivors"]
    fk = trace[1]["filter_killer"]
    last = 256 * ((L - 1) // 256)
    assert (fk >= last).sum() >= 300 and (fk[L:L + 300] == 0).all() and (fk[L + 300:L + 600] == L - 1).all()
    assert ((fk[:256] >= 0) & (fk[:256] < 256)).all()          # the first block of candidates dies in the first LDS batch
    assert (fk[256:512] < 0).sum() == 0 if L >= 512 else True
    print(f"filter: landmarks at the start of pass 2 == {L}; block 0 killed by batch 0 of {last // 256 + 1}; "
          f"{(fk >= last).sum()} candidates killed only by the last batch")


def test_distance_cases():
    c, idx, trace = R.traced("lattice at r")
    assert _passes(trace) == [(1, 26, 27)]
    c, idx, trace = R.traced("lattice under r")
    assert trace[0]["end"] < 27 and (trace[0]["pass_killer"] >= 0).any()
    P = c["points"].astype(np.float64)
    d = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
    assert np.nextafter(np.float32(0.25), np.float32(0)) == d[d > 0].min() < 0.25
    for i, (a, b, d) in enumerate(R.rounding_pairs()):
        assert d["fma_xy"] < d["numpy"] and d["fma_yx"] < d["numpy"] and d["assoc"] < d["numpy"]
        c, idx, trace = R.traced(f"rounding pair {i}")
        k = 2 + i % 2
        assert len(trace) == k + 1 and trace[k]["radius"] == d["numpy"]
        # at exactly d_np the pair is not near: b (index 1) is taken, the point behind it (index 2) is not
        assert list(idx) == [0, 3, 4, 1]
        # with any of the other roundings b is near a at that radius, and the pick would end with index 2
        P = c["points"].astype(np.float64)
        assert np.sqrt(((P[2] - P[0]) ** 2).sum()) > d["numpy"] * 1.03 and np.sqrt(((P[2] - P[1]) ** 2).sum()) < d["numpy"] / 8
        print(f"rounding pair {i}: numpy {d['numpy']!r} == r; fma {d['fma_xy']!r}, {d['fma_yx']!r} and other association "
              f"{d['assoc']!r} are < r")


def test_duplicates_and_long_pass_cases():
    dup = R.duplicates_case()
    assert len(np.unique(dup["points"].astype(np.float64), axis=0)) == dup["distinct"] == dup["num"]
    assert np.signbit(dup["points"][5, 0]) and not np.signbit(dup["points"][4, 0])
    c, idx, trace = R.traced("duplicates")
    assert not set(idx) & set(dup["losers"])
    c, idx, trace = R.traced("long pass count")
    assert 95 <= len(trace) <= 110 and trace[0]["survivors"] == 0 and sorted(idx) == list(range(6))
    print(f"long pass count: {len(trace)} passes, {sum(t['survivors'] == 0 for t in trace)} of them empty")
