"""Feature-TSDF fusion on the MI355X at the ties and edges: the integration bit for bit against the reference's own f32 volumes on
the exact scenes (tests/golden/fusion_edges.npz: every voxel, no mask), the surface bit for bit on dyadic volumes (ties at i + 0.5,
voxels at the level, -0.0, NaN, one-voxel axes, scan-tile sizes, the full checkerboard), the grid-stride minimum / maximum and the
three-kernel scan on one volume above 4 194 304 voxels, and the extract entry point's M contract with guard regions."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fusion_reference as R

pytestmark = pytest.mark.gpu
KEYS = ("tsdf", "weight", "color", "feat")


@pytest.fixture(scope="module")
def fx():
    return R.edges_fixture()


def _volume(sc):
    from splatloc_amd.fusion import TSDFVolume
    vol = TSDFVolume(torch.tensor(sc["dims"], dtype=torch.float64), torch.from_numpy(np.asarray(sc["origin"], np.float64)),
                     sc["voxel_size"], sc["feat_dim"], margin=sc["margin"])
    for t, a in zip(vol._axis, sc["axes"]):
        assert np.array_equal(t.cpu().numpy(), a)
    assert np.float32(vol.sdf_trunc) == np.float32(sc["sdf_trunc"])
    return vol


def _inputs(sc, frames=slice(None)):
    cuda = lambda a: torch.from_numpy(a[frames]).cuda()   # noqa: E731
    return cuda(sc["depth"]), cuda(sc["color"]), cuda(sc["feat"]), torch.from_numpy(sc["K"]), torch.from_numpy(sc["poses"][frames])


def _got(vol):
    tsdf, color, weight, feat = (t.cpu().numpy() for t in vol.get_volume())
    n = tsdf.size
    return {"tsdf": tsdf.reshape(n), "weight": weight.reshape(n), "color": color.reshape(n, 3), "feat": feat.reshape(n, -1)}


def _expected(fx, name):
    return {"tsdf": fx[f"{name}_tsdf"], "weight": fx[f"{name}_weight"], "color": fx[f"{name}_color"].astype(np.float32),
            "feat": fx[f"{name}_feat"]}


def _assert_bit_equal(got, want, what):
    assert np.array_equal(got["weight"], want["weight"]), f"{what}: weight"
    for k in KEYS:
        assert got[k].dtype == want[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k)
        bad = ~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} elements, first at {np.argwhere(bad)[0].tolist()}"
        assert np.array_equal(got[k], want[k], equal_nan=True)


@pytest.mark.parametrize("name", list(R.EDGE_SCENES))
def test_exact_scene_bit_for_bit_against_the_reference(name, fx):
    """C in {4, 8, 252}, obs_weight in {0.5, 1, 2, 3}; each scene as single integrate calls, as one launch of 8, split 3 + 5, and
    as 11 frames (8 + 3: the extra frames against integrate_f32 continued from the fixture)"""
    sc = R.edge_scene(name, frames=11)
    obs = sc["obs_weight"]
    assert np.array_equal(torch.inverse(torch.from_numpy(sc["poses"][:8]).float()).numpy(), fx[f"{name}_w2c"])   # the pose check
    want = _expected(fx, name)
    vol = _volume(sc)
    depth, color, feat, K, poses = _inputs(sc)
    for f in range(8):
        vol.integrate(depth[f], color[f], feat[f], K, poses[f], obs)
    _assert_bit_equal(_got(vol), want, f"{name}, single frames")
    vol.reset()
    vol.integrate_frames(depth[:8], color[:8], feat[:8], K, poses[:8], obs)
    _assert_bit_equal(_got(vol), want, f"{name}, one launch of 8")
    vol.reset()
    vol.integrate_frames(depth[:3], color[:3], feat[:3], K, poses[:3], obs)
    vol.integrate_frames(depth[3:8], color[3:8], feat[3:8], K, poses[3:8], obs)
    _assert_bit_equal(_got(vol), want, f"{name}, 3 + 5")
    vol.reset()
    vol.integrate_frames(depth, color, feat, K, poses, obs)
    more = R.integrate_scene_f32(sc, state={k: want[k].copy() for k in KEYS}, first=8)
    assert not np.array_equal(more["weight"], want["weight"])
    _assert_bit_equal(_got(vol), more, f"{name}, 11 frames")


def test_less_than_a_wave_and_the_smallest_image():
    """27 voxels under the axis scene's cameras, and a 1 x 1 image (pixel coordinates -0.5 and 0.5 both round to pixel 0) over the
    axis scene's volume, against integrate_f32"""
    sc = R.edge_scene("axis")
    small = dict(sc, dims=(3, 3, 3), origin=np.array([0.75, -0.125, 0.875]))
    small["axes"] = R.edge_axes(small["dims"], small["origin"], small["voxel_size"])
    vol = _volume(small)
    vol.integrate_frames(*_inputs(small))
    want = R.integrate_scene_f32(small)
    assert 5 < (want["weight"] > 0).sum() < 27 and want["weight"].max() >= 2
    _assert_bit_equal(_got(vol), want, "27 voxels")

    one = dict(sc, depth=sc["depth"][:, 4:5, 3:4].copy(), color=sc["color"][:, 4:5, 3:4].copy(), feat=sc["feat"][:, 4:5, 3:4].copy(),
               K=np.array([[4, 0, 0], [0, 4, 0], [0, 0, 1]], np.float32))
    one["depth"][0], one["depth"][3], one["depth"][6] = 4.0, 1.0, np.inf
    vol = _volume(one)
    vol.integrate_frames(*_inputs(one))
    counts = {}
    want = R.integrate_scene_f32(one, counts=counts)
    assert counts["px_low"] > 0 and counts["py_low"] > 0 and counts["px_high"] > 0 and counts["py_high"] > 0 and counts["updates"] > 20
    _assert_bit_equal(_got(vol), want, "1 x 1 image")


# ---- surface -------------------------------------------------------------------------------------------------------------------
def _loaded(tsdf, seed, feat_dim=4, voxel_size=0.125, origin=(0.5, -1.0, 2.0), payload=None):
    from splatloc_amd.fusion import TSDFVolume
    dims = tsdf.shape
    vol = TSDFVolume(torch.tensor(dims, dtype=torch.float64), torch.tensor(origin, dtype=torch.float64), voxel_size, feat_dim)
    color, feat = R.surface_payload(dims, seed, feat_dim) if payload is None else payload
    vol.load_state({"tsdf": torch.from_numpy(tsdf), "weight": torch.ones(dims), "color": torch.from_numpy(color),
                    "feat": torch.from_numpy(feat)})
    return vol, color, feat


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", list(R.surface_cases()))
def test_surface_bit_for_bit_on_exact_volumes(name):
    case = R.surface_cases()[name]
    vol, color, feat = _loaded(case["tsdf"], case["seed"])
    ref = R.surface_numpy(case["tsdf"], color, feat, level=case["level"], voxel_size=vol.voxel_size, origin=vol.origin.numpy())
    s = {k: v.cpu().numpy() for k, v in vol.surface(case["level"]).items()}
    assert _same_bits(np.float32(s["level"]), np.float32(ref["level"]))
    assert s["verts"].shape == (case["count"], 3)
    assert _same_bits(s["verts"], ref["verts"]) and _same_bits(s["points"], ref["points"])
    assert _same_bits(s["index"], ref["index"]) and _same_bits(s["colors"], ref["colors"]) and _same_bits(s["feats"], ref["feats"])
    assert int(np.isnan(s["verts"]).any(axis=1).sum()) >= case["nans"]


def test_surface_above_the_one_pass_scan_and_one_minmax_sweep():
    """(129, 128, 256) = 4 227 072 voxels (C = 4, 152 MB): the scan takes its three-kernel path (more than 2048 tiles of 2048) and
    every block of the minimum / maximum reduction strides 17 times (1024 x 256 voxels per sweep).  A clipped plane; the maximum
    sits in the last voxel and the minimum beyond the first sweep, so level None depends on both.  Order, index, colours and
    features exact, positions within one ulp.  Skips only when the device has less than 1.5 x the need free."""
    from splatloc_amd import fusion as F
    dims = (129, 128, 256)
    n = dims[0] * dims[1] * dims[2]
    assert n > 2048 * 2048 and n > 16 * 1024 * 256
    vb, sb = F.volume_bytes(dims, 4)
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * (vb + sb):
        pytest.skip(f"{free} bytes free, the test needs 1.5 x {vb + sb}")
    i, j, k = np.meshgrid(*[np.arange(d, dtype=np.float32) for d in dims], indexing="ij", sparse=True)
    tsdf = np.clip((np.float32(0.31) * i + np.float32(0.17) * j + np.float32(0.05) * k - np.float32(40.3)) * np.float32(0.25), -1, 1)
    tsdf = np.ascontiguousarray(tsdf, np.float32)
    tsdf.reshape(-1)[n - 1] = 3.0                       # the maximum: the last voxel
    tsdf.reshape(-1)[1024 * 256 + 777] = -2.5           # the minimum: second sweep of the reduction
    lin = np.arange(n, dtype=np.int64)[:, None]
    color = ((lin * 3 + np.arange(3)) % 255).astype(np.float32).reshape(*dims, 3) + np.float32(0.75)
    feat = (((lin * 4 + np.arange(4)) % 65).astype(np.float32).reshape(*dims, 4) - np.float32(32)) / np.float32(8)
    vol, color, feat = _loaded(tsdf, 21, payload=(color, feat))
    for level, want in ((None, 0.25), (0.0, 0.0)):
        ref = R.surface_numpy(tsdf, color, feat, level=level, voxel_size=vol.voxel_size, origin=vol.origin.numpy())
        s = {k: v.cpu().numpy() for k, v in vol.surface(level).items()}
        assert float(s["level"]) == float(ref["level"]) == want
        m = ref["verts"].shape[0]
        assert 20000 < m < 200000 and s["verts"].shape == (m, 3)
        assert ref["edge"][:, 0].min() > 2048 * 128 and ref["edge"][:, 0].max() > 2048 * 2048     # offsets from beyond tile 2048
        assert (np.abs(s["verts"] - ref["verts"]) <= np.spacing(np.abs(ref["verts"]))).all()
        assert np.array_equal(s["index"], ref["index"]) and np.array_equal(s["colors"], ref["colors"])
        assert np.array_equal(s["feats"], ref["feats"])
        pts = (s["verts"] * np.float32(vol.voxel_size)).astype(np.float64) + vol.origin.numpy()
        assert np.array_equal(s["points"], pts)


def test_extract_writes_m_rows_and_nothing_beyond():
    """splatraster_fusion_surface_extract through ctypes, a guard region after every output buffer: M below the counted total
    writes the first M vertices only; M above it writes the total, leaves index = -1 and the feature rows untouched beyond it;
    M = 0 writes nothing; M > 3 N is refused"""
    from splatloc_amd import _native
    case = R.surface_cases()["dyadic_level_0"]
    vol, color, feat = _loaded(case["tsdf"], case["seed"])
    ref = R.surface_numpy(case["tsdf"], color, feat, level=0.0, voxel_size=vol.voxel_size, origin=vol.origin.numpy())
    total, k, guard, Cf = case["count"], 37, 64, vol.feat_dim
    n = case["tsdf"].size
    lib, v = _native.load(), vol._native()
    ws = torch.empty(vol.surface_bytes, dtype=torch.uint8, device="cuda")
    counted = C.c_int64(0)
    assert lib.splatraster_fusion_surface_count(C.byref(v), 1, 0.0, ws.data_ptr(), C.byref(counted), None) == 0
    assert counted.value == total
    origin = (C.c_double * 3)(*vol.origin.tolist())
    rows = total + k + guard
    spec = {"verts": (torch.float32, 3, -7.0), "points": (torch.float64, 3, -7.0), "index": (torch.int64, 1, -7),
            "colors": (torch.uint8, 3, 0xA5), "feats": (torch.float32, Cf, -7.0)}

    def run(M):
        out = {key: torch.full((rows, w), fill, dtype=dt, device="cuda") for key, (dt, w, fill) in spec.items()}
        st = lib.splatraster_fusion_surface_extract(C.byref(v), ws.data_ptr(), vol.voxel_size, C.cast(origin, C.c_void_p), M,
                                                    *[out[key].data_ptr() for key in spec], None)
        torch.cuda.synchronize()
        return st, {key: t.cpu().numpy() for key, t in out.items()}

    def untouched(out, keys, start):
        return all((out[key][start:] == spec[key][2]).all() for key in keys)

    want = {"verts": ref["verts"], "points": ref["points"], "index": ref["index"][:, None], "colors": ref["colors"], "feats": ref["feats"]}
    st, out = run(total - k)
    assert st == 0 and all(np.array_equal(out[key][:total - k], want[key][:total - k]) for key in spec)
    assert untouched(out, spec, total - k)
    st, out = run(total + k)
    assert st == 0 and all(np.array_equal(out[key][:total], want[key]) for key in spec)
    assert (out["index"][total:total + k] == -1).all() and untouched(out, ("index",), total + k)
    assert untouched(out, ("verts", "points", "colors", "feats"), total)
    st, out = run(total)
    assert st == 0 and all(np.array_equal(out[key][:total], want[key]) for key in spec) and untouched(out, spec, total)
    st, out = run(0)
    assert st == 0 and untouched(out, spec, 0)
    st, out = run(3 * n + 1)
    assert st == 1 and untouched(out, spec, 0)
    st, out = run(-1)
    assert st == 1 and untouched(out, spec, 0)
