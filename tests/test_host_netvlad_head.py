"""tests/netvlad_reference.py held to itself, and the host side of the NetVLAD head (csrc/netvlad_head.hip, splatloc_amd/netvlad.py),
without a GPU: the float32 restatement in hloc's literal form lies inside the bars of the float64 oracle on every case (so the
bars are ones the reference alone stays within), every builder reaches the edge it names, every wrong model fails its case, the
exact family is exact, the retrieval case keeps its margin, and the C entries refuse bad arguments before any launch."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from tests import netvlad_reference as R


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_lies_inside_the_bars(name):
    r = R.ratios(name, R.restatement(R.case(name)))
    print(name, {k: round(v, 4) for k, v in r.items()})
    assert r and R.within(r), r


def test_assign_rule_rests_on_a_restatement_error():
    """the 4x rule needs an error to take four times of: positive wherever the arithmetic rounds at all"""
    for name in R.HEAD_CASES:
        c = R.case(name)
        _, _, ea, ei = R.assign_reference(name)
        K, D = c["score_w"].shape
        assert ea < 1e-5 and ei < 1e-5, (name, ea, ei)
        if not c.get("exact") and K > 1:
            assert ea > 0, name
        if not c.get("exact") and D > 1 and name != "saturated":
            assert ei > 0, name


def test_builders_reach_their_edges():
    T, DT, SL, OT, BT = R.T, R.D_TILE, R.I_SLICE, R.O_TILE, R.B_TILE
    heads = [R.case(n) for n in R.HEAD_CASES]
    shapes = [(c["features"].shape, c["score_w"].shape[0], 0 if c["whiten_w"] is None else c["whiten_w"].shape[0]) for c in heads]
    assert {s[0][2] for s in shapes} >= {1, T - 1, T, T + 1, 2 * T + 1, 1200}
    assert {s[0][1] for s in shapes} >= {1, 3, DT - 1, DT, DT + 1, 512}
    assert {s[1] for s in shapes} >= {1, 2, 63, 64}
    assert {s[2] for s in shapes} >= {0, 1, OT - 1, OT, OT + 1}
    assert {s[0][0] for s in shapes} >= {1, 2, BT, BT + 1}
    projs = [R.case(n) for n in R.PROJECT_CASES]
    assert {c["whiten_w"].shape[1] for c in projs} >= {1, 3, SL - 1, SL, SL + 1, 2 * SL + 4}
    assert {c["x"].shape[0] for c in projs} >= {1, 2, BT, BT + 1}
    assert any(c["unaligned"] and c["whiten_w"].shape[1] % 4 == 0 for c in projs)          # only the base makes it the scalar path
    assert any(c["whiten_w"].shape[1] % 4 == 0 and not c["unaligned"] for c in projs)
    assert {c["score_b"] is None for c in heads} == {True, False} and {c["intranorm"] for c in heads} == {True, False}
    assert {c["whiten_b"] is None for c in heads if c["whiten_w"] is not None} == {True, False}
    lay = R.case("layer")
    assert tuple(lay["features"].shape[1:]) == (512, 1200) and tuple(lay["whiten_w"].shape) == (128, 512 * 64)

    z = R.case("zero_locations")
    o = R.oracle_of("zero_locations")
    soft = torch.softmax(z["score_b"].double(), 0)
    for b, n in z["zero"]:
        assert not z["features"][b, :, n].any() and o["inv_norm"][b, n] == 1.0 / R.EPS
        assert torch.allclose(o["assign"][b, :, n], soft, rtol=0, atol=1e-15)
    zi = R.case("zero_image")
    assert not zi["features"][1].any() and zi["features"][0].any() and zi["features"][2].any()
    assert float(R.oracle_of("zero_image")["v"][1].norm()) == pytest.approx(1.0)               # -centers sum a, normalised

    s = R.case("saturated")
    a = R.oracle_of("saturated")["assign"][0]
    logits = torch.einsum("kd,dn->kn", s["score_w"].double(), torch.nn.functional.normalize(s["features"][0].double(), dim=0))
    onehot = (logits.max(0).values >= 79.0) & (logits.min(0).values <= -79.0)
    assert onehot.sum() >= 16 and bool(((a[:, onehot].max(0).values == 1.0) & (a[:, onehot].sum(0) == 1.0)).all())
    assert (logits.max(0).values < -90).sum() >= 16 and (logits.min(0).values > 88.8).sum() >= 16


@pytest.mark.parametrize("name", sorted(R.WRONG))
def test_every_wrong_model_fails_its_case(name):
    ratio = R.wrong_output(name)
    print(name, R.WRONG[name], ratio)
    assert ratio > 1.0, (name, ratio)


@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_family_is_exact(name):
    c = R.case(name)
    r, o = R.restatement(c), R.oracle_of(name)
    keys = ("assign", "inv_norm", "raw") if "features" in c else ("y_raw",)
    for k in keys:
        assert torch.equal(o[k], o[k].float().double()), k                  # the oracle's value is a float32
        assert R.same_bits(r[k], o[k].float()), k
    if "features" in c:
        K = c["score_w"].shape[0]
        assert bool((r["assign"] == 1.0 / K).all())
        # the raw V through the whitening, flags 0: exact as well
        y = R.project64(r["raw"], c["whiten_w"], c["whiten_b"], 0)["y"]
        assert torch.equal(y, y.float().double())
        assert R.same_bits(torch.nn.functional.linear(r["raw"], c["whiten_w"], c["whiten_b"]), y.float())


def test_retrieval_case_keeps_its_margin():
    idx, gap, bar = R.retrieval_margin()
    c = R.case("retrieval")
    print(f"smallest gap {gap:.3g}, descriptor bar {bar:.3g}, ratio {gap / bar:.1f}")
    assert gap >= 64.0 * bar > 0.0
    assert idx.tolist() == [[3 * q, 3 * q + 1, 3 * q + 2] for q in range(idx.shape[0])] and c["topk"] == 3     # by growing noise


def _lib():
    from splatloc_amd import _native
    return _native, _native.load()


def test_abi_version_is_still_20_and_the_tiles_are_the_cases():
    native, lib = _lib()
    assert native.ABI_VERSION == 20 and lib.splatraster_abi_version() == 20
    from splatloc_amd import netvlad
    assert netvlad.tiles() == R.TILES
    v = [C.c_int32(0) for _ in range(5)]
    for i in range(5):
        args = [C.byref(x) for x in v]
        args[i] = None
        assert lib.splatraster_netvlad_tiles(*args) == 1


def test_workspace_bytes_behaves_as_documented():
    _, lib = _lib()
    nb = C.c_size_t(7)

    def ws(B, D, K, N, O):
        nb.value = 7
        st = lib.splatraster_netvlad_workspace_size(B, D, K, N, O, C.byref(nb))
        return st, nb.value

    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert ws(8, 512, 64, 1200, 4096) == (0, up(16 * 8 * 4096 * 4))             # 32768 / 2048 slices of partial sums
    assert ws(1, 3, 2, 1, 1) == (0, 256) and ws(2, 1025, 2, 5, 3) == (0, up(2 * 2 * 3 * 4))     # I = 2050: two slices
    assert ws(0, 512, 64, 1200, 4096) == (0, 0)
    for bad in ((-1, 4, 2, 5, 3), (1, 0, 2, 5, 3), (1, 4, 0, 5, 3), (1, 4, 65, 5, 3), (1, 4, 2, 0, 3), (1, 4, 2, 5, 0),
                (1, 1 << 25, 64, 5, 3)):
        assert ws(*bad) == (1, 0), bad
    assert lib.splatraster_netvlad_workspace_size(1, 4, 2, 5, 3, None) == 1


def test_argument_checks_come_before_any_launch():
    _, lib = _lib()
    BAD = 1
    fake = C.c_void_p(1 << 12)            # never dereferenced: validation comes first
    odd = C.c_void_p((1 << 12) + 2)

    def assign(B=2, D=8, K=4, N=70, f=fake, w=fake, b=fake, a=fake, inv=fake, ws=None, nb=0):
        return lib.splatraster_netvlad_assign(B, D, K, N, f, w, b, a, inv, ws, nb, None)

    assert assign(B=-1) == BAD and assign(D=0) == BAD and assign(K=0) == BAD and assign(K=65) == BAD and assign(N=0) == BAD
    assert assign(D=1 << 25, K=64) == BAD                                   # D K = 2^31
    assert all(assign(**{k: None}) == BAD for k in ("f", "w", "a", "inv"))
    assert all(assign(**{k: odd}) == BAD for k in ("f", "w", "b", "a", "inv", "ws"))
    assert assign(B=0) == 0 and assign(B=0, f=None, a=None, inv=None) == 0   # nothing to launch

    def aggregate(B=2, D=8, K=4, N=70, f=fake, a=fake, inv=fake, c=fake, flags=3, v=fake, ws=None, nb=0):
        return lib.splatraster_netvlad_aggregate(B, D, K, N, f, a, inv, c, flags, v, ws, nb, None)

    assert aggregate(B=-1) == BAD and aggregate(D=0) == BAD and aggregate(K=0) == BAD and aggregate(K=65) == BAD and aggregate(N=0) == BAD
    assert aggregate(flags=4) == BAD and aggregate(flags=-1) == BAD
    assert all(aggregate(**{k: None}) == BAD for k in ("f", "a", "inv", "c", "v"))
    assert all(aggregate(**{k: odd}) == BAD for k in ("f", "a", "inv", "c", "v", "ws"))
    assert aggregate(B=0) == 0

    nb = C.c_size_t(0)
    assert lib.splatraster_netvlad_workspace_size(2, 1025, 2, 5, 3, C.byref(nb)) == 0
    need = nb.value

    def project(B=2, O=3, I=2050, x=fake, w=fake, b=fake, flags=2, y=fake, ws=fake, nbytes=need):
        return lib.splatraster_netvlad_project(B, O, I, x, w, b, flags, y, ws, nbytes, None)

    assert project(B=-1) == BAD and project(O=0) == BAD and project(I=0) == BAD and project(flags=1) == BAD and project(flags=4) == BAD
    assert all(project(**{k: None}) == BAD for k in ("x", "w", "y", "ws"))
    assert all(project(**{k: odd}) == BAD for k in ("x", "w", "b", "y", "ws"))
    assert project(nbytes=need - 1) == BAD and project(nbytes=0) == BAD      # a workspace that is too small
    assert project(B=0) == 0


def test_host_queries_never_initialise_the_device():
    """the tile and workspace queries answer in a process that can see no device at all"""
    native, _ = _lib()
    code = ("import ctypes as C, sys\n"
            "lib = C.CDLL(sys.argv[1])\n"
            "v = [C.c_int32(0) for _ in range(5)]\n"
            "n = C.c_size_t(0)\n"
            "assert lib.splatraster_netvlad_tiles(*[C.byref(x) for x in v]) == 0\n"
            "assert lib.splatraster_netvlad_workspace_size(8, 512, 64, 1200, 4096, C.byref(n)) == 0 and n.value > 0\n"
            "print(*[x.value for x in v])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, native.lib_path()], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == list(R.TILES.values())


def test_python_layer_refuses_before_device_work():
    from splatloc_amd import netvlad as NV
    w, c = torch.zeros(4, 8), torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NV.NetVLADHead(w, c)
    with pytest.raises(ValueError):
        NV.NetVLADHead(w.numpy(), c)
    assert NV.MAX_K == 64 and NV.INTRANORM == R.INTRANORM and NV.L2NORM == R.L2NORM
