"""Host side of the feature-TSDF fusion: grid arithmetic and axis tables against the reference's, the C ABI's sizing and argument
validation (before any HIP call), the feat_dim rules, the memory guard's arithmetic, the float64 restatement against the golden
volumes, and the numpy vertex rule on an analytic sphere.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fusion_reference as R


@pytest.mark.parametrize("name", list(R.SCENES))
def test_grid_and_axis_tables_are_bit_identical_to_the_reference(name):
    from splatloc_amd import fusion as F
    fx, cfg = R.fixture(name), R.SCENES[name]
    voxel_dim, origin = F.grid_from_bounds(cfg["bounds"], cfg["voxel_size"])
    assert voxel_dim.dtype == origin.dtype == torch.float64
    assert np.array_equal(voxel_dim.numpy(), fx["voxel_dim"]) and np.array_equal(origin.numpy(), fx["origin"])
    assert F._dims(voxel_dim) == fx["dims"].tolist()
    tables = F.axis_tables(voxel_dim, origin, cfg["voxel_size"])
    for t, k in zip(tables, ("axis_x", "axis_y", "axis_z")):
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), fx[k])
    assert cfg["margin"] * float(cfg["voxel_size"]) == float(fx["sdf_trunc"])


def test_office_0_grid_is_the_issue_s():
    from splatloc_amd import fusion as F
    voxel_dim, origin = F.grid_from_bounds([[-3, 3], [-4, 2.5], [-2, 2.5]], 0.02)
    assert F._dims(voxel_dim) == [300, 325, 225]
    vb, sb = F.volume_bytes(voxel_dim, 256)
    n = 300 * 325 * 225
    assert n * 256 > 2 ** 32                                    # element offsets of the feature volume need 64 bits
    assert vb == n * 4 * (1 + 1 + 3 + 256) == 22_902_750_000
    assert n * 4 <= sb < n * 4 + (1 << 20)


def test_sizing_function_and_bad_arguments():
    from splatloc_amd import _native
    lib = _native.load()
    vb, sb = C.c_size_t(7), C.c_size_t(7)
    assert lib.splatraster_fusion_bytes(50, 40, 30, 8, C.byref(vb), C.byref(sb)) == 0
    assert vb.value == 60000 * 4 * 13 and sb.value >= 60000 * 4 and sb.value % 256 == 0
    for bad in ((0, 40, 30, 8), (50, -1, 30, 8), (50, 40, 30, 0), (50, 40, 30, 6), (50, 40, 30, 260), (50, 40, 30, -4),
                (1 << 11, 1 << 10, 1 << 10, 8), (1 << 30, 1 << 30, 4, 8)):
        vb.value = sb.value = 7
        assert lib.splatraster_fusion_bytes(*bad, C.byref(vb), C.byref(sb)) == 1, bad
        assert vb.value == 0 and sb.value == 0
    assert lib.splatraster_fusion_bytes(50, 40, 30, 8, None, C.byref(sb)) == 1
    assert lib.splatraster_fusion_bytes(1 << 10, 1 << 10, 1 << 10, 256, C.byref(vb), C.byref(sb)) == 0    # exactly 2^30 voxels
    assert vb.value == (1 << 30) * 4 * 261

    # null volume / null pointers / oversized arguments: BAD_ARG before any HIP call (no device is present here)
    n = C.c_int64(5)
    assert lib.splatraster_fusion_integrate(None, 1, 60, 80, *([None] * 5), 1.0, 0.06, None) == 1
    assert lib.splatraster_fusion_surface_count(None, 0, 0.0, None, C.byref(n), None) == 1 and n.value == 0
    assert lib.splatraster_fusion_surface_extract(None, None, 0.02, None, 0, *([None] * 5), None) == 1
    v = _native.FusionVolume()
    v.dim[0], v.dim[1], v.dim[2], v.feat_dim = 50, 40, 30, 8
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *([None] * 5), 1.0, 0.06, None) == 1    # null volumes
    fake = 1 << 12            # never dereferenced: validation comes first
    v.tsdf = v.weight = v.color = v.feat = fake
    v.axis[0] = v.axis[1] = v.axis[2] = fake
    ptrs = [C.c_void_p(fake)] * 5
    assert lib.splatraster_fusion_integrate(C.byref(v), 0, 60, 80, *([None] * 5), 1.0, 0.06, None) == 0   # no frames: nothing to do
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *([None] * 5), 1.0, 0.06, None) == 1   # null images
    assert lib.splatraster_fusion_integrate(C.byref(v), 9, 60, 80, *ptrs, 1.0, 0.06, None) == 1           # more than 8 frames
    assert lib.splatraster_fusion_integrate(C.byref(v), -1, 60, 80, *ptrs, 1.0, 0.06, None) == 1
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 0, 80, *ptrs, 1.0, 0.06, None) == 1
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 1 << 16, *ptrs, 1.0, 0.06, None) == 1      # oversized image
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *ptrs, 1.0, 0.0, None) == 1            # truncation must be > 0
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *ptrs, float("nan"), 0.06, None) == 1
    v.feat = fake + 4
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *ptrs, 1.0, 0.06, None) == 1           # rows not 16-byte aligned
    v.feat, v.feat_dim = fake, 6
    assert lib.splatraster_fusion_integrate(C.byref(v), 1, 60, 80, *ptrs, 1.0, 0.06, None) == 1
    v.feat_dim = 8
    assert lib.splatraster_fusion_surface_count(C.byref(v), 0, 0.0, None, C.byref(n), None) == 1          # null workspace
    assert lib.splatraster_fusion_surface_count(C.byref(v), 1, float("nan"), C.c_void_p(fake), C.byref(n), None) == 1
    assert lib.splatraster_fusion_surface_count(C.byref(v), 0, 0.0, C.c_void_p(fake), None, None) == 1
    origin = (C.c_double * 3)(0, 0, 0)
    assert lib.splatraster_fusion_surface_extract(C.byref(v), C.c_void_p(fake), 0.02, origin, -1, *ptrs, None) == 1
    assert lib.splatraster_fusion_surface_extract(C.byref(v), C.c_void_p(fake), 0.02, origin, 3 * 60000 + 1, *ptrs, None) == 1
    assert lib.splatraster_fusion_surface_extract(C.byref(v), C.c_void_p(fake), 0.02, None, 4, *ptrs, None) == 1
    assert lib.splatraster_fusion_surface_extract(C.byref(v), C.c_void_p(fake), 0.02, origin, 4, *([None] * 5), None) == 1


@pytest.mark.parametrize("feat_dim", [0, 2, 3, 6, 255, 260, 512, -4, 8.5])
def test_unsupported_feat_dim_raises_value_error(feat_dim):
    from splatloc_amd import fusion as F
    with pytest.raises(ValueError, match="feat_dim"):
        F.check_feat_dim(feat_dim)
    with pytest.raises(ValueError, match="feat_dim"):
        F.TSDFVolume(torch.tensor([4.0, 4.0, 4.0]), torch.zeros(3, dtype=torch.float64), 0.02, feat_dim)


def test_argument_validation_needs_no_device():
    from splatloc_amd import fusion as F
    assert [F.check_feat_dim(c) for c in (4, 64, 256)] == [4, 64, 256]
    with pytest.raises(ValueError, match="voxel_dim"):
        F.TSDFVolume(torch.tensor([4.0, 4.0]), torch.zeros(3), 0.02, 8)
    with pytest.raises(ValueError, match="voxel_dim"):
        F.TSDFVolume(torch.tensor([4.0, 0.5, 4.0]), torch.zeros(3), 0.02, 8)
    with pytest.raises(ValueError, match="2\\^30"):
        F.TSDFVolume(torch.tensor([2048.0, 1024.0, 1024.0]), torch.zeros(3), 0.02, 8)
    with pytest.raises(ValueError, match="voxel_size"):
        F.TSDFVolume(torch.tensor([4.0, 4.0, 4.0]), torch.zeros(3), 0.0, 8)
    with pytest.raises(ValueError, match="origin"):
        F.TSDFVolume(torch.tensor([4.0, 4.0, 4.0]), torch.zeros(2), 0.02, 8)
    with pytest.raises(ValueError, match="bounds"):
        F.grid_from_bounds([[0, 1], [0, 1]])
    # the volume lives on the device: a CPU device is refused, there is no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.TSDFVolume(torch.tensor([4.0, 4.0, 4.0]), torch.zeros(3, dtype=torch.float64), 0.02, 8, device="cpu")


def test_memory_guard_arithmetic():
    from splatloc_amd import fusion as F
    need, _ = F.volume_bytes([300, 325, 225], 256)
    assert need == 22_902_750_000 and 300 * 325 * 225 * 256 > 2 ** 32
    F.check_memory(need, need)                 # exactly enough is enough
    with pytest.raises(RuntimeError, match=r"needs 22902750000 bytes \(21\.33 GiB\).*22902749999 bytes"):
        F.check_memory(need, need - 1)
    with pytest.raises(RuntimeError, match="the surface workspace needs 10 bytes"):
        F.check_memory(10, 0, "the surface workspace")


@pytest.mark.parametrize("name", list(R.SCENES))
def test_restatement_reproduces_the_golden(name):
    """the float64 restatement on the stored inputs against the reference's f32 volumes: its deviations over the decided voxels stay
    within the recorded maxima (one part in 10^6 of slack for another numpy's summation order), the weights agree exactly, and the
    exclusions stay under the 1 % cap"""
    fx, cfg = R.fixture(name), R.SCENES[name]
    dims, Cf = fx["dims"].tolist(), int(fx["feat_dim"])
    N = int(np.prod(dims))
    p = R.centres([fx["axis_x"], fx["axis_y"], fx["axis_z"]])
    color_im, feat_im = R.images(name)
    state = R.fresh_state(N, Cf)
    undecided, tie, updated = np.zeros(N, bool), np.zeros((N, 3), bool), np.zeros(N, bool)
    for f in range(R.FRAMES):
        diag = {}
        R.integrate_f64(p, state, fx["depth"][f], color_im[f], feat_im[f], fx["K"], fx["w2c"][f], 1.0, float(fx["sdf_trunc"]), diag)
        undecided |= diag["undecided"]
        tie |= diag["tie"]
        updated |= diag["valid"]
    ok = ~undecided
    assert np.array_equal(undecided, fx["undecided"])
    assert np.array_equal(tie & (updated & ok)[:, None], fx["tie"])
    assert abs(fx["excluded"][0] - undecided.mean()) < 1e-12 and undecided.mean() <= 0.01 and fx["excluded"][1] <= 0.01
    assert np.array_equal(fx["weight"][ok].astype(np.float64), state["weight"][ok])
    slack = 1 + 1e-6
    assert np.abs(fx["tsdf"].astype(np.float64) - state["tsdf"])[ok].max() <= slack * float(fx["dev_tsdf"]) < 1e-5
    col_ok = ok[:, None] & ~fx["tie"]
    assert np.abs(fx["color"].astype(np.float64) - state["color"])[col_ok].max() <= float(fx["dev_color"]) == 0.0
    s = fx["sample_idx"]
    assert not undecided[s].any()
    assert np.abs(fx["sample_feat"].astype(np.float64) - state["feat"][s]).max() <= slack * float(fx["dev_feat"]) < 1e-6
    assert np.abs(fx["featsum"] - state["feat"].sum(axis=1))[ok].max() <= slack * float(fx["dev_featsum"]) + 1e-12
    # the reproduced quirks are in the data: negative feature components were clamped to 0, free space was averaged
    assert state["feat"].min() == 0.0 and fx["sample_feat"].min() == 0.0 and R.images(name)[1].min() < -0.39
    assert ((fx["tsdf"] == 1.0) & (fx["weight"] > 0)).any()
    # and the surface has material
    surf = R.surface_numpy(fx["tsdf"].reshape(dims))
    assert surf["verts"].shape[0] == int(fx["crossing_edges"]) > 5000


def test_vertex_rule_on_an_analytic_sphere():
    dims, centre, radius = (24, 20, 22), (11.3, 9.6, 10.2), 7.25
    sdf = R.sphere_sdf(dims, centre, radius)
    color = np.random.default_rng(0).random((*dims, 3), dtype=np.float32) * 255
    feat = np.random.default_rng(1).random((*dims, 4), dtype=np.float32)
    origin = np.array([-1.0, 0.5, 2.0])
    s = R.surface_numpy(sdf, color, feat, level=0.0, voxel_size=0.02, origin=origin)
    # as many vertices as sign-changing edges, counted independently
    neg = sdf < 0
    edges = (neg[1:] != neg[:-1]).sum() + (neg[:, 1:] != neg[:, :-1]).sum() + (neg[:, :, 1:] != neg[:, :, :-1]).sum()
    assert s["verts"].shape[0] == edges > 500
    # every vertex within half a voxel diagonal of the sphere
    d = np.sqrt(((s["verts"].astype(np.float64) - np.array(centre)) ** 2).sum(axis=1)) - radius
    assert np.abs(d).max() < 0.5 * np.sqrt(3.0)
    assert np.abs(d).max() < 0.05          # linear interpolation of a distance field does far better than the bound
    # order: ascending (voxel, axis); each vertex lies on its edge; index is the nearer end
    key = s["edge"][:, 0] * 3 + s["edge"][:, 1]
    assert (np.diff(key) > 0).all()
    ijk = np.stack(np.unravel_index(s["edge"][:, 0], dims), axis=1)
    off = s["verts"] - ijk
    for ax in range(3):
        sel = s["edge"][:, 1] == ax
        assert (off[sel][:, ax] >= 0).all() and (off[sel][:, ax] <= 1).all()
        assert (np.delete(off[sel], ax, axis=1) == 0).all()
    r = np.stack(np.unravel_index(s["index"], dims), axis=1)
    assert np.abs(r - s["verts"]).max() <= 0.5
    assert np.array_equal(s["colors"], np.floor(color.reshape(-1, 3)[s["index"]]).astype(np.uint8))
    assert np.array_equal(s["feats"], feat.reshape(-1, 4)[s["index"]])
    assert np.allclose(s["points"], s["verts"].astype(np.float64) * 0.02 + origin, atol=1e-6)
    # the default level is the mid-range of the field
    assert R.surface_numpy(sdf)["level"] == np.float32(0.5) * (sdf.min() + sdf.max())


def test_import_opens_no_device():
    import subprocess
    import sys
    import os
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = ("import torch, splatloc_amd.fusion as F; F.volume_bytes([8, 8, 8], 16); "
            "assert not torch.cuda.is_initialized(); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["ok"], r.stderr[-800:]
