"""The surface mesh on the MI355X: faces and normals bit for bit against tests/mesh_reference.py on every builder, at the scan-tile
cell counts, on one-voxel axes, the full checkerboard and two volumes above the one-pass scan; the invariants of a closed oriented
mesh on the device's own output; determinism; the extract entry point's F / M contract with guard regions; get_mesh / save_mesh."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fusion_reference as R
from tests import mesh_reference as M

pytestmark = pytest.mark.gpu
SURFACE_KEYS = ("verts", "points", "index", "colors", "feats")


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


def _reference(tsdf, color, feat, level, vol):
    surface = R.surface_numpy(tsdf, color, feat, level=level, voxel_size=vol.voxel_size, origin=vol.origin.numpy())
    return M.mesh_numpy(tsdf, level, surface=surface)


def _check(tsdf, level, seed=5):
    """mesh() against the reference, bit for bit in every key; returns (device output as numpy, reference)"""
    vol, color, feat = _loaded(tsdf, seed)
    ref = _reference(tsdf, color, feat, level, vol)
    got = {k: v.cpu().numpy() for k, v in vol.mesh(level).items()}
    assert _same_bits(np.float32(got["level"]), np.float32(ref["level"]))
    for k in SURFACE_KEYS:
        assert _same_bits(got[k], ref[k]), k
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["faces"].shape
    bad = np.nonzero((got["faces"] != ref["faces"]).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {ref['faces'].shape[0]} faces differ, first {bad[0]}: {got['faces'][bad[0]]} / {ref['faces'][bad[0]]}"
    assert got["normals"].dtype == np.float32 and got["normals"].shape == ref["normals"].shape
    bad = np.nonzero((got["normals"].view(np.uint32) != ref["normals"].view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {ref['normals'].shape[0]} normals differ, first {bad[0]}: {got['normals'][bad[0]]} / "
                           f"{ref['normals'][bad[0]]}")
    return got, ref


@pytest.mark.parametrize("name", list(M.cases()))
def test_mesh_bit_for_bit_and_invariants_on_the_device_s_output(name):
    case = M.cases()[name]
    got, _ = _check(case["tsdf"], case["level"])
    n, faces = got["verts"].shape[0], got["faces"]
    assert faces.shape[0] > 300 and faces.min() >= 0 and faces.max() < n
    assert M.duplicate_edges(faces) == 0 and M.used_vertices(n, faces).all()
    if case["closed"]:
        assert M.closed_and_oriented(faces)
    if case["euler"] is not None:
        assert M.euler(n, faces) == case["euler"]
    if name == "sphere":
        fn = M.face_normals(got["verts"], faces)
        for k in range(3):
            assert ((fn * got["normals"][faces[:, k]]).sum(axis=1) > 0).all()


@pytest.mark.parametrize("dims, cells", [((24, 90, 2), 2047), ((9, 17, 17), 2048), ((684, 2, 4), 2049)])
def test_cell_counts_around_one_scan_tile(dims, cells):
    assert (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) == cells
    got, _ = _check(R.dyadic_volume(dims, 19, neg_zero=True), 0.0)
    assert got["faces"].shape[0] > cells // 2


@pytest.mark.parametrize("dims", [(1, 9, 8), (7, 1, 9), (8, 9, 1), (1, 1, 70), (70, 1, 1), (1, 1, 1)])
def test_one_voxel_axes_have_vertices_and_normals_but_no_face(dims):
    tsdf = R.dyadic_volume(dims, 23, zeros=False) if max(dims) > 1 else np.full(dims, -1.0, np.float32)
    got, ref = _check(tsdf, 0.0)
    assert got["faces"].shape == (0, 3) and got["normals"].shape == got["verts"].shape
    if max(dims) > 1:
        assert got["verts"].shape[0] >= 10
        one = [a for a in range(3) if dims[a] == 1]
        assert (got["normals"][:, one] == 0).all() and (np.abs(got["normals"]).sum(axis=1) > 0).any()
    else:
        assert got["verts"].shape[0] == 0


def test_full_checkerboard():
    X, Y, Z = 31, 32, 30
    got, _ = _check(R.checkerboard((X, Y, Z)), 0.0)
    assert got["faces"].shape[0] == 4 * (X - 1) * (Y - 1) * (Z - 1)        # cases 0x69 and 0x96: four corners cut off
    assert M.duplicate_edges(got["faces"]) == 0


@pytest.mark.parametrize("dims", [(129, 128, 256), (130, 129, 257)])
def test_above_the_one_pass_scan(dims):
    """(129, 128, 256): the vertex offsets come from the three-kernel scan, the 4 145 280 cells are the largest one-pass scan of the
    suite (2025 tiles); (130, 129, 257): 4 227 072 cells, the face offsets take the three-kernel scan too.  A clipped plane and two
    far voxels that make level None depend on the whole volume.  The surface outputs are compared as the existing large surface
    test compares them (verts within one ulp, points from the device's verts, index, colours and features exactly); faces and
    normals exactly.  About 150 MB of device memory."""
    from splatloc_amd import _native
    n, cells = dims[0] * dims[1] * dims[2], (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    lib = _native.load()
    assert lib.splatraster_debug_scan_path(n) == 2
    assert lib.splatraster_debug_scan_path(cells) == (2 if dims[0] == 130 else 1)
    i, j, k = np.meshgrid(*[np.arange(d, dtype=np.float32) for d in dims], indexing="ij", sparse=True)
    tsdf = np.clip((np.float32(0.31) * i + np.float32(0.17) * j + np.float32(0.05) * k - np.float32(40.3)) * np.float32(0.25), -1, 1)
    tsdf = np.ascontiguousarray(tsdf, np.float32)
    tsdf.reshape(-1)[n - 1] = 3.0
    tsdf.reshape(-1)[1024 * 256 + 777] = -2.5
    lin = np.arange(n, dtype=np.int64)[:, None]
    color = ((lin * 3 + np.arange(3)) % 255).astype(np.float32).reshape(*dims, 3) + np.float32(0.75)
    feat = (((lin * 4 + np.arange(4)) % 65).astype(np.float32).reshape(*dims, 4) - np.float32(32)) / np.float32(8)
    vol, _, _ = _loaded(tsdf, 21, payload=(color, feat))
    for level, want in ((None, 0.25), (0.0, 0.0)):
        ref = _reference(tsdf, color, feat, level, vol)
        got = {key: v.cpu().numpy() for key, v in vol.mesh(level).items()}
        assert float(got["level"]) == float(ref["level"]) == want
        m = ref["verts"].shape[0]
        assert 20000 < m < 200000 and got["verts"].shape == (m, 3)
        assert ref["edge"][:, 0].max() > 2048 * 2048
        assert (np.abs(got["verts"] - ref["verts"]) <= np.spacing(np.abs(ref["verts"]))).all()
        assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["colors"], ref["colors"])
        assert np.array_equal(got["feats"], ref["feats"])
        assert np.array_equal(got["points"], (got["verts"] * np.float32(vol.voxel_size)).astype(np.float64) + vol.origin.numpy())
        assert ref["faces"].shape[0] > m and np.array_equal(got["faces"], ref["faces"])
        assert M.duplicate_edges(got["faces"]) == 0 and M.used_vertices(m, got["faces"]).all()
        assert np.array_equal(got["normals"].view(np.uint32), ref["normals"].view(np.uint32))


def test_two_runs_give_identical_bytes():
    case = M.cases()["random_2"]
    vol, _, _ = _loaded(case["tsdf"], 5)
    a = {k: v.cpu().numpy().tobytes() for k, v in vol.mesh(0.0).items()}
    b = {k: v.cpu().numpy().tobytes() for k, v in vol.mesh(0.0).items()}
    assert a == b and len(a["faces"]) > 0


def test_extract_writes_f_faces_m_normals_and_nothing_beyond():
    """splatraster_fusion_mesh_extract through ctypes, a guard region after both outputs: F (M) below the counted total writes the
    first F (M) rows only; above it the counted rows, faces -1 up to F, normals untouched beyond the total; 0 writes nothing; F >
    5 cells, M > 3 voxels and negative counts are refused and write nothing"""
    from splatloc_amd import _native
    case = M.cases()["random_1"]
    tsdf = case["tsdf"]
    vol, color, feat = _loaded(tsdf, 7)
    ref = _reference(tsdf, color, feat, 0.0, vol)
    tm, tf, k, guard = ref["verts"].shape[0], ref["faces"].shape[0], 29, 64
    voxels, cells = tsdf.size, int(np.prod([d - 1 for d in tsdf.shape]))
    lib, v = _native.load(), vol._native()
    ws = torch.empty(vol.surface_bytes, dtype=torch.uint8, device="cuda")
    nb = C.c_size_t(0)
    assert lib.splatraster_fusion_mesh_bytes(*tsdf.shape, C.byref(nb)) == 0
    mws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    counted = C.c_int64(0)
    assert lib.splatraster_fusion_surface_count(C.byref(v), 1, 0.0, ws.data_ptr(), C.byref(counted), None) == 0 and counted.value == tm
    assert lib.splatraster_fusion_mesh_count(C.byref(v), ws.data_ptr(), mws.data_ptr(), C.byref(counted), None) == 0
    assert counted.value == tf
    FILL_F, FILL_N = -7, -7.0

    def run(m, f):
        faces = torch.full((tf + k + guard, 3), FILL_F, dtype=torch.int32, device="cuda")
        normals = torch.full((tm + k + guard, 3), FILL_N, dtype=torch.float32, device="cuda")
        st = lib.splatraster_fusion_mesh_extract(C.byref(v), ws.data_ptr(), mws.data_ptr(), m, f, faces.data_ptr(), normals.data_ptr(),
                                                 None)
        torch.cuda.synchronize()
        return st, faces.cpu().numpy(), normals.cpu().numpy()

    st, faces, normals = run(tm - k, tf - k)
    assert st == 0 and np.array_equal(faces[:tf - k], ref["faces"][:tf - k]) and (faces[tf - k:] == FILL_F).all()
    assert np.array_equal(normals[:tm - k], ref["normals"][:tm - k]) and (normals[tm - k:] == FILL_N).all()
    st, faces, normals = run(tm + k, tf + k)
    assert st == 0 and np.array_equal(faces[:tf], ref["faces"]) and (faces[tf:tf + k] == -1).all() and (faces[tf + k:] == FILL_F).all()
    assert np.array_equal(normals[:tm], ref["normals"]) and (normals[tm:] == FILL_N).all()
    st, faces, normals = run(tm, tf)
    assert st == 0 and np.array_equal(faces[:tf], ref["faces"]) and (faces[tf:] == FILL_F).all()
    assert np.array_equal(normals[:tm], ref["normals"]) and (normals[tm:] == FILL_N).all()
    st, faces, normals = run(tm, 0)
    assert st == 0 and (faces == FILL_F).all() and np.array_equal(normals[:tm], ref["normals"])
    st, faces, normals = run(0, tf)
    assert st == 0 and np.array_equal(faces[:tf], ref["faces"]) and (normals == FILL_N).all()
    for m, f in ((0, 0), (tm, 5 * cells + 1), (3 * voxels + 1, tf), (-1, tf), (tm, -1)):
        st, faces, normals = run(m, f)
        assert st == (0 if (m, f) == (0, 0) else 1) and (faces == FILL_F).all() and (normals == FILL_N).all(), (m, f)
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), ws.data_ptr(), mws.data_ptr(), tm, tf, None, None, None) == 1


def test_get_mesh_and_save_mesh(tmp_path):
    case = M.cases()["torus"]
    tsdf = case["tsdf"]
    vol, color, feat = _loaded(tsdf, 9, feat_dim=8)
    ref = _reference(tsdf, color, feat, 0.0, vol)
    verts, faces, norms, colors, feats = vol.get_mesh(0.0)
    m, f = ref["verts"].shape[0], ref["faces"].shape[0]
    assert all(isinstance(a, np.ndarray) for a in (verts, faces, norms, colors, feats))
    assert (verts.dtype, verts.shape) == (np.float64, (m, 3)) and (faces.dtype, faces.shape) == (np.int32, (f, 3))
    assert (norms.dtype, norms.shape) == (np.float32, (m, 3)) and (colors.dtype, colors.shape) == (np.uint8, (m, 3))
    assert (feats.dtype, feats.shape) == (np.float32, (m, 8))
    assert np.array_equal(verts, ref["points"]) and np.array_equal(faces, ref["faces"]) and np.array_equal(feats, ref["feats"])
    ply, npy = tmp_path / "out" / "mesh.ply", tmp_path / "out" / "feat_cloud.npy"
    assert vol.save_mesh(ply, npy, level=0.0) == (m, f)
    lines = ply.read_text().split("\n")
    assert lines[2] == f"element vertex {m}" and lines[12] == f"element face {f}" and lines[14] == "end_header"
    assert len(lines) == 15 + m + f + 1 and lines[-1] == ""
    row = lambda i: "%f %f %f %f %f %f %d %d %d" % (*verts[i], *norms[i], *colors[i])   # noqa: E731
    assert lines[15] == row(0) and lines[15 + m - 1] == row(m - 1)
    assert lines[15 + m] == "3 %d %d %d" % tuple(faces[0]) and lines[-2] == "3 %d %d %d" % tuple(faces[-1])
    assert np.array_equal(np.load(npy), feats)
    assert vol.save_mesh(tmp_path / "only.ply", level=0.0) == (m, f) and not (tmp_path / "feat_cloud.npy").exists()
