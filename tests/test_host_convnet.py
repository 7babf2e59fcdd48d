"""tests/convnet_reference.py held to itself, and the host side of the convolution backbones (csrc/conv2d.hip,
splatloc_amd/convnet.py), without a GPU: every builder reaches the edge it names, the float32 model of the declared chain lies inside
the derived bars on every case and equals torch's CPU float32 layer bit for bit on the exact family, the closed forms are what the
reference computes, every wrong model fails its case, the C entries refuse bad arguments before any device work, and the layer tables
produce the documented shapes."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from tests import convnet_reference as R


def _lib():
    from splatloc_amd import _native
    return _native, _native.load()


def test_abi_version_is_still_20_and_the_tiles_are_the_cases():
    native, lib = _lib()
    assert native.ABI_VERSION == 20 and lib.splatraster_abi_version() == 20          # new symbols only
    from splatloc_amd import convnet
    assert convnet.tiles() == R.TILES
    assert R.ROWS % 2 == 0 and R.COLS % 2 == 0                                       # a pool window never straddles a tile
    v = [C.c_int32(0) for _ in range(4)]
    for i in range(4):
        args = [C.byref(x) for x in v]
        args[i] = None
        assert lib.splatraster_conv2d_tiles(*args) == 1


def test_builders_reach_their_edges():
    CO, ROWS, COLS, CI = R.CO, R.ROWS, R.COLS, R.CI
    cases = [R.case(n) for n in R.CASES]
    assert {c["w"].shape[1] for c in cases} >= {1, 3, CI - 1, CI, CI + 1, 2 * CI + 1, 256, 512}
    assert {c["w"].shape[0] for c in cases} >= {1, CO - 1, CO, CO + 1, 65}
    sizes = {(tuple(c["x"].shape[2:]), c["pool"]) for c in cases}
    assert sizes >= {((1, 1), False), ((1, COLS + 1), False), ((ROWS + 1, 1), False), ((2, 2), True), ((3, 3), True),
                     ((2 * ROWS + 1, 37), False), ((2 * ROWS + 1, 37), True)}
    assert 37 % 4 != 0 and 37 > COLS                      # a row that is not float4-aligned, more than one tile of columns
    k1 = R.case("k1_256_65_5x7")
    assert tuple(k1["w"].shape) == (65, 256, 1, 1) and tuple(k1["x"].shape[2:]) == (5, 7)
    b3 = R.case("batch3")["x"]
    assert b3.shape[0] == 3 and not torch.equal(b3[0], b3[1]) and not torch.equal(b3[1], b3[2])
    assert {c["b"] is None for c in cases} == {True, False} and {c["relu"] for c in cases} == {True, False}
    for n in R.EXACT_CASES:
        c = R.case(n)
        assert c.get("exact") and torch.equal(c["w"], c["w"].round())
        if n.startswith("exact_"):
            assert torch.equal(c["x"], c["x"].round())
            assert float(c["x"].abs().max()) <= 8 and float(c["w"].abs().max()) <= 4 and 9 * c["w"].shape[1] * 32 + 16 < 2 ** 24
    f = R.preprocess_frame()
    assert bool((f < 0).any()) and bool((f > 1).any()) and bool((f == 0).any()) and bool((f == 1).any())
    # the pooled float case has windows whose maximum is not their first element, and negative maxima without ReLU
    c = R.case("hw_2rows_p1x37_pool_norelu")
    assert bool((R.oracle(*R.layer_args(c)) < 0).any())


@pytest.mark.parametrize("name", R.CASES)
def test_model_lies_inside_the_bars(name):
    c = R.case(name)
    r = R.ratio(R.model32(*R.layer_args(c)), *R.layer_args(c))
    print(name, round(r, 4))
    assert r <= 1.0


@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_family_is_exact(name):
    c = R.case(name)
    want = R.expected_exact(name)
    assert R.same_bits(R.model32(*R.layer_args(c)), want)
    assert torch.equal(want.double(), R.oracle(*R.layer_args(c)))            # and it is the float64 oracle's value
    if name in ("ones", "corner_impulses", "zero_weights"):
        assert R.same_bits(want, R.closed_form(name))


def test_closed_forms_say_what_they_should():
    ones = R.closed_form("ones")
    cin = R.case("ones")["x"].shape[1]
    assert ones[0, 0, 0, 0] == 4 * cin and ones[0, 0, 0, 1] == 6 * cin and ones[0, 0, 1, 0] == 6 * cin and ones[0, 0, 1, 1] == 9 * cin
    assert ones[0, 0, -1, -1] == 4 * cin
    imp = R.closed_form("corner_impulses")
    # around the top-left impulse: out[y, x] is the tap (1 - y, 1 - x)
    assert imp[0, 0, 0, 0] == 5 and imp[0, 0, 0, 1] == 4 and imp[0, 0, 1, 0] == 2 and imp[0, 0, 1, 1] == 1
    # around the bottom-right one: out[H - 1 - dy, W - 1 - dx] is the tap (1 + dy, 1 + dx)
    assert imp[0, 0, -1, -1] == 5 and imp[0, 0, -1, -2] == 6 and imp[0, 0, -2, -1] == 8 and imp[0, 0, -2, -2] == 9
    z = R.closed_form("zero_weights")
    assert bool((z >= 0).all()) and bool((z[:, :, 0, 0] == z[:, :, 3, 2]).all())


@pytest.mark.parametrize("name", sorted(R.WRONG))
def test_every_wrong_model_fails_its_case(name):
    assert R.wrong_fails(name), (name, R.WRONG[name])


def test_preprocess_reference_rounds_operation_by_operation():
    x = R.preprocess_frame()
    y = R.preprocess32(x)
    mean = torch.tensor(R.MEAN, dtype=torch.float32)
    assert bool((y[:, :, 0, 0] == -mean).all()) and bool((y[:, :, 1, 0] == -mean).all())                  # 0 and below
    assert bool((y[:, :, 0, 1] == 255.0 - mean).all()) and bool((y[:, :, 1, 1] == 255.0 - mean).all())    # 1 and above
    assert R.same_bits(y, ((x.double() * 255.0).float().clamp(0, 255).double() - mean.double().view(1, 3, 1, 1)).float())


def test_argument_checks_come_before_any_device_work():
    _, lib = _lib()
    BAD = 1
    fake = C.c_void_p(1 << 12)            # never dereferenced: validation comes first
    odd = C.c_void_p((1 << 12) + 2)

    def conv(B=2, Cin=3, Cout=4, H=5, W=6, k=3, x=fake, w=fake, b=fake, flags=3, out=fake, ws=None, nb=0):
        return lib.splatraster_conv2d(B, Cin, Cout, H, W, k, x, w, b, flags, out, ws, nb, None)

    assert conv(B=-1) == BAD and conv(Cin=0) == BAD and conv(Cout=0) == BAD and conv(H=0) == BAD and conv(W=0) == BAD
    assert conv(H=1, flags=2) == BAD and conv(W=1, flags=2) == BAD and conv(H=1, W=1, flags=3) == BAD     # nothing to pool
    assert all(conv(k=k) == BAD for k in (0, 2, 4, 5, -1))
    assert conv(flags=4) == BAD and conv(flags=-1) == BAD and conv(flags=8 | 1) == BAD
    assert conv(Cin=1 << 16, H=1 << 8, W=1 << 7) == BAD and conv(Cout=1 << 16, H=1 << 8, W=1 << 7) == BAD     # 2^31 elements per image
    assert conv(Cin=1, Cout=1, H=1 << 14, W=1 << 14) == BAD                                                  # a chunk's planes
    assert all(conv(**{k: None}) == BAD for k in ("x", "w", "out"))
    assert all(conv(**{k: odd}) == BAD for k in ("x", "w", "b", "out", "ws"))
    assert conv(B=0) == 0 and conv(B=0, x=None, w=None, out=None) == 0       # nothing to launch
    assert conv(B=0, k=2) == BAD                                             # but still a layer

    def pre(B=2, H=5, W=6, rgb=fake, out=fake):
        return lib.splatraster_netvlad_preprocess(B, H, W, rgb, out, None)

    assert pre(B=-1) == BAD and pre(H=0) == BAD and pre(W=0) == BAD and pre(H=1 << 15, W=1 << 15) == BAD
    assert pre(rgb=None) == BAD and pre(out=None) == BAD and pre(rgb=odd) == BAD and pre(out=odd) == BAD
    assert pre(B=0) == 0 and pre(B=0, rgb=None, out=None) == 0


def test_host_queries_never_initialise_the_device():
    """the tile query and the refusals answer in a process that can see no device at all"""
    native, _ = _lib()
    code = ("import ctypes as C, sys\n"
            "lib = C.CDLL(sys.argv[1])\n"
            "v = [C.c_int32(0) for _ in range(4)]\n"
            "assert lib.splatraster_conv2d_tiles(*[C.byref(x) for x in v]) == 0\n"
            "assert lib.splatraster_conv2d(1, 3, 4, 5, 6, 2, None, None, None, 0, None, None, 0, None) == 1\n"
            "print(*[x.value for x in v])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, native.lib_path()], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == list(R.TILES.values())


@pytest.mark.parametrize("hw", ((8, 8), (9, 9), (15, 15), (16, 16), (24, 40), (8, 15), (16, 9)))
def test_layer_tables_produce_the_documented_shapes(hw):
    from splatloc_amd import convnet as CN
    h, w = hw
    sp = CN.superpoint_shapes(h, w)
    assert [n for n, _, _ in sp] == list(CN.SUPERPOINT_WIDTHS)
    assert sp[0][1:] == (h, w) and sp[1][1:] == (h // 2, w // 2) and sp[3][1:] == (h // 4, w // 4)
    assert all(s[1:] == (h // 8, w // 8) for s in sp[5:])                    # floor at every pool: 15 -> 7 -> 3 -> 1
    assert (15 // 2 // 2 // 2, 9 // 2 // 2 // 2) == (1, 1) and ((h // 2) // 2) // 2 == h // 8
    if min(h, w) >= 16:
        vg = CN.vgg16_shapes(h, w)
        assert [i for i, _, _ in vg] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
        assert vg[0][1:] == (h, w) and vg[1][1:] == (h // 2, w // 2) and vg[-1][1:] == (h // 16, w // 16)
    pools = [i for i, _, _, p in CN.VGG16_CONVS if p]
    assert pools == [2, 7, 14, 21] and [n for n, p in CN.SUPERPOINT_ENCODER if p] == ["conv1b", "conv2b", "conv3b"]
    widths = [(ci, co) for _, ci, co, _ in CN.VGG16_CONVS]
    assert widths[0] == (3, 64) and widths[-1] == (512, 512) and all(a[1] == b[0] for a, b in zip(widths, widths[1:]))
    sw = CN.SUPERPOINT_WIDTHS
    assert sw["conv1a"] == (1, 64) and sw["convPb"] == (256, 65) and sw["convDb"] == (256, 256) and sw["convPa"] == sw["convDa"] == (128, 256)


def test_python_layer_refuses_before_device_work():
    from splatloc_amd import convnet as CN
    x, w = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CN.conv2d(x, w)
    with pytest.raises(ValueError):
        CN.conv2d(x.numpy(), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CN.preprocess(x)
    assert CN.RELU == 1 and CN.POOL2 == 2
    sd = R.superpoint_state_dict()
    assert set(sd) == {f"{n}.{p}" for n in CN.SUPERPOINT_WIDTHS for p in ("weight", "bias")}
    assert set(R.vgg16_state_dict()) == {f"backbone.{i}.{p}" for i, _, _, _ in CN.VGG16_CONVS for p in ("weight", "bias")}
