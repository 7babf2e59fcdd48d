"""The device convolution backbones (splatloc_amd/convnet.py, csrc/conv2d.hip) against tests/convnet_reference.py.

Every layer case runs through splatraster_conv2d into sentinel-filled buffers with a lead and a guard.  The exact family and the
three closed forms are held bit for bit; the seeded float cases within the derived elementwise bar gamma(9 Cin + 1) * (conv64(|x|,
|w|) + |b|); a pooled output equals max_pool2d of the device's own unpooled output bit for bit; an image of a batch of three equals
its own run bit for bit, and two runs are bit-identical.  The whole networks run on He-initialised seeded weights, every layer
checked on the device's own output of the layer before, within that layer's bar.

Measured on the MI355X, error / bar (the bound is 1): cin1 0.257 (the worst: nine terms), fused_preprocess 0.071, cout_tile_m1 0.063,
cout_tile 0.062, cout_tile_p1 0.057, cin3 0.055, the other float cases 0.001 (k1_256_65_5x7) to 0.039; the SuperPoint encoder's
conv1a 0.273, its other layers 0.001 to 0.007; the VGG16 trunk's first layer 0.149, the others 0.001 to 0.007; 0 on the exact family.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from splatloc_amd import _native, convnet as CN, localize, netvlad as NV, superpoint
from splatloc_amd._host import _stream
from tests import convnet_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD          # a NaN no kernel computes
GUARD = 256
LEAD = 64


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


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def run_layer(x, w, b, relu, pool):
    """device tensors in, the checked device output out"""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = _Out(B, Cout, Ho, Wo, lead=LEAD)
    st = _native.load().splatraster_conv2d(B, Cin, Cout, H, W, k, _p(x), _p(w), _p(b), (1 if relu else 0) | (2 if pool else 0), _p(out.t),
                                           None, 0, _stream(x.device))
    assert st == 0
    return out.done()


@functools.lru_cache(maxsize=None)
def device_run(name):
    x, w, b, relu, pool = R.layer_args(R.case(name))
    y = run_layer(_dev(x), _dev(w), _dev(b), relu, pool)
    torch.cuda.synchronize()
    return y.cpu()


def test_the_cases_were_built_for_the_device_tiles():
    assert CN.tiles() == R.TILES


@pytest.mark.parametrize("name", R.FLOAT_CASES)
def test_float_cases_within_the_bar(name):
    r = R.ratio(device_run(name), *R.layer_args(R.case(name)))
    print(name, round(r, 4))
    assert r <= 1.0


@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_family_and_closed_forms_bit_for_bit(name):
    y = device_run(name)
    assert R.same_bits(y, R.expected_exact(name))
    if not name.startswith("exact_"):
        assert R.same_bits(y, R.closed_form(name))


@pytest.mark.parametrize("name", ("hw_2x2_pool", "hw_3x3_pool", "hw_2rows_p1x37_pool", "hw_2rows_p1x37_pool_norelu", "k1_3_2_pool", "batch3_pool",
                                  "exact_2rows_p1x37_pool"))
def test_pooled_output_is_the_pool_of_the_unpooled_one(name):
    x, w, b, relu, pool = R.layer_args(R.case(name))
    assert pool
    full = run_layer(_dev(x), _dev(w), _dev(b), relu, False)
    assert R.same_bits(device_run(name), F.max_pool2d(full.cpu(), 2))


@pytest.mark.parametrize("name", ("batch3", "batch3_pool", "exact_batch3"))
def test_an_image_does_not_depend_on_the_batch(name):
    x, w, b, relu, pool = R.layer_args(R.case(name))
    full = device_run(name)
    assert x.shape[0] == 3
    for i in range(3):
        one = run_layer(_dev(x[i:i + 1]), _dev(w), _dev(b), relu, pool)
        assert R.same_bits(one.cpu()[0], full[i]), i


@pytest.mark.parametrize("name", ("hw_2rows_p1x37", "batch3_pool", "k1_256_65_5x7"))
def test_repeat_runs_are_bit_identical(name):
    first = device_run(name)
    device_run.cache_clear()
    second = device_run(name)
    assert first is not second and R.same_bits(first, second)


def test_unaligned_weights_take_the_scalar_loads_to_the_same_bits():
    """Cin a multiple of the chunk: float4 weight loads from an aligned base, scalar loads from a base 4 bytes off; one chain"""
    x, w, b, relu, pool = R.layer_args(R.case("cin_chunk"))
    flat = torch.empty(w.numel() + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(w.shape)
    view.copy_(w)
    assert view.data_ptr() % 16 == 4 and w.shape[1] % R.CI == 0
    assert R.same_bits(run_layer(_dev(x), view, _dev(b), relu, pool).cpu(), device_run("cin_chunk"))


def test_python_conv2d_is_the_entry_and_b0_launches_nothing():
    x, w, b, relu, pool = R.layer_args(R.case("hw_2rows_p1x37_pool"))
    y = CN.conv2d(_dev(x), _dev(w), _dev(b), relu=relu, pool=pool)
    assert R.same_bits(y.cpu(), device_run("hw_2rows_p1x37_pool"))
    assert tuple(CN.conv2d(torch.zeros(0, 9, 5, 6, device="cuda"), _dev(w), _dev(b)).shape) == (0, 35, 5, 6)
    with pytest.raises(ValueError):
        CN.conv2d(_dev(x), _dev(w)[:, :3].contiguous())
    with pytest.raises(ValueError):
        CN.conv2d(_dev(x)[:, :, :1], _dev(w), pool=True)


def test_preprocess_bit_for_bit():
    x = R.preprocess_frame()
    out, xd = _Out(*x.shape, lead=LEAD), x.cuda()
    st = _native.load().splatraster_netvlad_preprocess(x.shape[0], x.shape[2], x.shape[3], _p(xd), _p(out.t), _stream(xd.device))
    assert st == 0
    want = R.preprocess32(x)
    assert R.same_bits(out.done().cpu(), want) and R.same_bits(CN.preprocess(xd).cpu(), want)


def _check_layers(taps, first, table):
    """every layer on the device's own output of the layer before, within that layer's bar"""
    x = first
    worst = {}
    for name, (w, b), relu, pool, src in table:
        xin = x if src is None else taps[src].cpu()
        y = taps[name].cpu()
        worst[name] = R.ratio(y, xin, w.cpu(), b.cpu(), relu, pool)
        x = y
    print({k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_superpoint_encoder_layer_by_layer():
    enc = CN.SuperPointEncoder(R.superpoint_state_dict())
    g = torch.Generator().manual_seed(61)
    image = torch.rand(2, 1, 24, 40, generator=g)
    taps = {}
    semi, coarse = enc(image.cuda(), taps)
    assert tuple(semi.shape) == (2, 65, 3, 5) and tuple(coarse.shape) == (2, 256, 3, 5)
    table = [(n, enc.params[n], True, pool, None) for n, pool in CN.SUPERPOINT_ENCODER]
    table += [("convPa", enc.params["convPa"], True, False, "conv4b"), ("convPb", enc.params["convPb"], False, False, None),
              ("convDa", enc.params["convDa"], True, False, "conv4b"), ("convDb", enc.params["convDb"], False, False, None)]
    _check_layers(taps, image, table)
    assert [tuple(taps[n].shape[2:]) for n, _, _ in CN.superpoint_shapes(24, 40)] == [(h, w) for _, h, w in CN.superpoint_shapes(24, 40)]
    again = enc(image.cuda())                                        # the cached buffers serve the next call
    assert R.same_bits(again[0].cpu(), semi.cpu()) and R.same_bits(again[1].cpu(), coarse.cpu())
    one = enc(image[1:].cuda())
    assert R.same_bits(one[0].cpu()[0], semi.cpu()[1]) and R.same_bits(one[1].cpu()[0], coarse.cpu()[1])
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 1, 7, 40, device="cuda"))
    assert tuple(enc(torch.rand(1, 1, 15, 9, device="cuda"))[0].shape) == (1, 65, 1, 1)


def test_superpoint_extractor_is_the_encoder_and_the_head():
    sd = R.superpoint_state_dict()
    ext = CN.SuperPointExtractor(sd, max_keypoints=64, keypoint_threshold=0.0005, remove_borders=2)
    g = torch.Generator().manual_seed(62)
    image = torch.rand(2, 1, 24, 40, generator=g).cuda()
    got = ext.detect(image)
    want = superpoint.detect(*ext.encoder(image), nms_radius=4, keypoint_threshold=0.0005, max_keypoints=64, remove_borders=2)
    assert got.keys() == want.keys()
    for k in got:
        assert torch.equal(got[k].cpu().view(torch.int32) if got[k].dtype is torch.float32 else got[k].cpu(),
                           want[k].cpu().view(torch.int32) if want[k].dtype is torch.float32 else want[k].cpu()), k
    post = ext.postprocess(image, original_size=(80, 48))
    assert len(post) == 2
    for d in post:
        n = d["keypoints"].shape[0]
        assert set(d) == {"keypoints", "scores", "descriptors", "dense_scores"}
        assert tuple(d["keypoints"].shape) == (n, 2) and tuple(d["scores"].shape) == (n,) and tuple(d["descriptors"].shape) == (256, n)
        assert tuple(d["dense_scores"].shape) == (24, 40)
    dense = ext.dense_descriptors(image, rows=(8, 16))
    assert tuple(dense.shape) == (2, 8, 40, 256)


def test_vgg16_trunk_layer_by_layer():
    trunk = CN.VGG16Trunk(R.vgg16_state_dict())
    g = torch.Generator().manual_seed(63)
    x = torch.randn(2, 3, 32, 48, generator=g) * 50.0
    taps = {}
    y = trunk(x.cuda(), taps)
    assert tuple(y.shape) == (2, 512, 2, 3)
    table = [(idx, trunk.params[idx], idx != 28, pool, None) for idx, _, _, pool in CN.VGG16_CONVS]
    _check_layers(taps, x, table)
    assert bool((taps[26] >= 0).all()) and bool((y < 0).any())        # ReLU behind every layer but the last
    assert R.same_bits(trunk(x.cuda()).cpu(), y.cpu())
    assert R.same_bits(trunk(x[:1].cuda()).cpu()[0], y.cpu()[0])


def test_netvlad_is_preprocess_trunk_and_head_and_feeds_retrieve():
    sd = dict(R.vgg16_state_dict(), **R.netvlad_head_state_dict(K=4, O=8))
    net = CN.NetVLAD(sd)
    g = torch.Generator().manual_seed(64)
    image = (torch.rand(3, 3, 32, 48, generator=g) * 1.2 - 0.1).cuda()
    y = net(image)
    head = NV.NetVLADHead.from_state_dict(sd)
    want = head(CN.VGG16Trunk(sd)(CN.preprocess(image)))
    assert tuple(y.shape) == (3, 8) and R.same_bits(y.cpu(), want.cpu())
    assert float((y.cpu().double().norm(dim=1) - 1).abs().max()) < 1e-5
    idx, sims = localize.retrieve(y[:1], y, k=2)
    assert int(idx[0, 0]) == 0 and float(sims[0, 0]) == pytest.approx(1.0, abs=1e-5)
    bare = CN.NetVLAD({k: v for k, v in sd.items() if not k.startswith("whiten.")})
    assert tuple(bare(image).shape) == (3, 512 * 4)
