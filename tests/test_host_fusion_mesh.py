"""The surface mesh without a GPU: the library's compile-time triangulation table against its numpy derivation and the stated
values, the test volumes (each reaches the edge it was built for), the invariants of the reference meshes, wrong models that must
break one of them, the new entry points' argument checks, and the PLY writer byte for byte against the reference's own output."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mesh_reference as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_write.ply")
ROTATED = [c for c in range(256) if any(M.fan_start(loop) for loop in M.case_loops(c))]
SEVEN = [c for c in range(256) if any(len(loop) == 7 for loop in M.case_loops(c))]


@pytest.fixture(scope="module")
def meshes():
    return {name: M.mesh_numpy(c["tsdf"], c["level"]) for name, c in M.cases().items()}


def _tris(table, case):
    row = table[case]
    return [tuple(int(e) for e in row[1 + 3 * t:4 + 3 * t]) for t in range(int(row[0]))]


def test_library_table_is_the_numpy_derivation_and_has_the_stated_values():
    from splatloc_amd import _native
    lib = _native.load()
    buf = np.full(4096, 0xAB, np.uint8)
    assert lib.splatraster_debug_mc_table(buf.ctypes.data_as(C.c_void_p)) == 0
    assert lib.splatraster_debug_mc_table(None) == 1
    table = buf.reshape(256, M.TABLE_ROW)
    assert np.array_equal(table, M.mc_table())
    count_crc, edge_crc, n_ids = M.table_crcs(table)
    assert (count_crc, edge_crc, n_ids) == (M.COUNT_CRC, M.EDGE_CRC, 2460)
    assert int(table[:, 0].max()) == 5 and int(table[:, 0].sum()) == 820
    assert np.bincount(table[:, 0], minlength=6).tolist() == M.HISTOGRAM
    for case in range(256):
        n = int(table[case, 0])
        assert (table[case, 1:1 + 3 * n] < 12).all() and (table[case, 1 + 3 * n:] == 0xFF).all()
    assert _tris(table, 0x01) == [(0, 4, 8)]
    assert _tris(table, 0x03) == [(4, 8, 9), (4, 9, 5)]
    assert _tris(table, 0x41) == [(0, 4, 8), (3, 6, 10)]
    assert _tris(table, 0xFE) == [(0, 8, 4)]
    assert _tris(table, 0x96) == [(0, 9, 5), (1, 10, 4), (2, 8, 6), (3, 11, 7)]


def test_derivation_edges_loops_and_rotations():
    assert M.edge_corners(0) == (0, 1) and M.edge_corners(5) == (1, 3) and M.edge_corners(11) == (3, 7)
    lengths = set()
    for case in range(256):
        below = {c for c in range(8) if case >> c & 1}
        loops = M.case_loops(case)
        lengths |= {len(loop) for loop in loops}
        crossing = {e for e in range(12) if len(below & set(M.edge_corners(e))) == 1}
        assert sorted(e for loop in loops for e in loop) == sorted(crossing)      # every crossing edge once, no other edge
        assert [loop[0] for loop in loops] == sorted(min(loop) for loop in loops)
    assert lengths == {3, 4, 5, 6, 7}
    assert len(ROTATED) == 18 and sum(M.fan_start(loop) != 0 for c in range(256) for loop in M.case_loops(c)) == 18


def test_every_builder_reaches_its_edge(meshes):
    def cells(name, which):
        return int(np.isin(meshes[name]["case"], which).sum())

    def ambiguous(name):
        return sum(M.ambiguous_faces(int(c)) for c in meshes[name]["case"].reshape(-1))

    for name in ("sphere", "two_spheres", "torus"):
        assert ambiguous(name) <= 10 and meshes[name]["faces"].shape[0] > 500          # smooth surfaces
    assert meshes["sphere"]["faces"].shape[0] == 520
    for seed in (1, 2, 3):
        for name in (f"random_{seed}", f"random_{seed}_negated"):
            assert ambiguous(name) >= 50 and cells(name, SEVEN) >= 3 and cells(name, ROTATED) >= 3, name
    assert ambiguous("padded_checkerboard") >= 600 and cells("padded_checkerboard", [0x69, 0x96]) == 125
    cases = meshes["all_cases"]["case"].reshape(-1)
    assert set(cases.tolist()) == set(range(256))
    assert cells("all_cases", ROTATED) >= 18 and cells("all_cases", SEVEN) >= len(SEVEN)
    for name in ("dyadic", "dyadic_mid_range", "dyadic_nan"):
        assert meshes[name]["faces"].shape[0] > 300 and M.unpaired_edges(meshes[name]["faces"]) > 0    # open at the border
    assert np.isnan(M.cases()["dyadic_nan"]["tsdf"]).sum() >= 30
    assert int((meshes["dyadic_nan"]["normals"] == 0).all(axis=1).sum()) >= 100      # NaN gradients give zero normals
    assert float(meshes["dyadic_mid_range"]["level"]) == 0.25


def test_reference_meshes_are_closed_oriented_and_complete(meshes):
    for name, case in M.cases().items():
        m = meshes[name]
        n, faces = m["verts"].shape[0], m["faces"]
        assert faces.dtype == np.int32 and m["normals"].dtype == np.float32 and m["normals"].shape == (n, 3)
        assert faces.shape[0] == int(M.mc_table()[m["case"].reshape(-1), 0].sum())
        assert M.duplicate_edges(faces) == 0, name                     # also on the open dyadic volumes
        assert M.used_vertices(n, faces).all(), name
        if case["closed"]:
            assert M.closed_and_oriented(faces), name
        if case["euler"] is not None:
            assert M.euler(n, faces) == case["euler"], name
        lens = np.sqrt((m["normals"].astype(np.float64) ** 2).sum(axis=1))
        assert (np.abs(lens[lens > 0] - 1) < 1e-6).all()


def test_sphere_faces_and_normals_point_out(meshes):
    m = meshes["sphere"]
    fn = M.face_normals(m["verts"], m["faces"])
    for k in range(3):
        assert ((fn * m["normals"][m["faces"][:, k]]).sum(axis=1) > 0).all()
    centre = np.array([5.3, 5.6, 5.45])
    assert ((m["normals"] * (m["verts"] - centre)).sum(axis=1) > 0).all()      # increasing TSDF: away from the centre


def test_wrong_models_break_an_invariant(meshes):
    r1 = M.cases()["random_1"]["tsdf"]
    assert M.duplicate_edges(M.mesh_numpy(r1, 0.0, table=M.mc_table(rotate=False))["faces"]) > 0
    assert M.duplicate_edges(meshes["random_1"]["faces"]) == 0
    flipped = M.mesh_numpy(r1, 0.0, table_odd=M.mc_table(flip=True))["faces"]
    assert M.unpaired_edges(flipped) > 0 and M.unpaired_edges(meshes["random_1"]["faces"]) == 0
    s = M.mesh_numpy(M.sphere(), 0.0, table=M.mc_table(reverse=True))
    assert M.closed_and_oriented(s["faces"])                                    # still closed: only the sphere test tells
    fn = M.face_normals(s["verts"], s["faces"])
    assert ((fn * s["normals"][s["faces"][:, 0]]).sum(axis=1) < 0).all()


def test_new_entry_points_refuse_bad_arguments_before_any_hip_call():
    from splatloc_amd import _native
    lib = _native.load()
    nb = C.c_size_t(7)
    assert lib.splatraster_fusion_mesh_bytes(50, 40, 30, C.byref(nb)) == 0
    assert nb.value >= 49 * 39 * 29 * 4 and nb.value % 256 == 0
    assert lib.splatraster_fusion_mesh_bytes(1, 40, 30, C.byref(nb)) == 0 and nb.value >= 256      # no cell: still a total
    for bad in ((0, 40, 30), (50, -1, 30), (1 << 11, 1 << 10, 1 << 10), (1 << 30, 1 << 30, 4)):
        nb.value = 7
        assert lib.splatraster_fusion_mesh_bytes(*bad, C.byref(nb)) == 1 and nb.value == 0, bad
    assert lib.splatraster_fusion_mesh_bytes(50, 40, 30, None) == 1
    nb.value = 7
    assert lib.splatraster_fusion_mesh_bytes(1 << 10, 1 << 10, 1 << 10, C.byref(nb)) == 4 and nb.value == 0   # 5 * 1023^3 >= 2^32
    assert lib.splatraster_fusion_mesh_bytes(950, 951, 952, C.byref(nb)) == 0                     # 5 * cells just below 2^32
    assert 5 * 949 * 950 * 951 < 1 << 32 <= 5 * 950 * 951 * 952

    n = C.c_int64(5)
    fake = C.c_void_p(1 << 12)            # never dereferenced: validation comes first
    assert lib.splatraster_fusion_mesh_count(None, fake, fake, C.byref(n), None) == 1 and n.value == 0
    assert lib.splatraster_fusion_mesh_extract(None, fake, fake, 0, 0, fake, fake, None) == 1
    v = _native.FusionVolume()
    v.dim[0], v.dim[1], v.dim[2], v.feat_dim = 50, 40, 30, 8
    assert lib.splatraster_fusion_mesh_count(C.byref(v), fake, fake, C.byref(n), None) == 1       # null volumes
    v.tsdf = v.weight = v.color = v.feat = 1 << 12
    assert lib.splatraster_fusion_mesh_count(C.byref(v), None, fake, C.byref(n), None) == 1
    assert lib.splatraster_fusion_mesh_count(C.byref(v), fake, None, C.byref(n), None) == 1
    assert lib.splatraster_fusion_mesh_count(C.byref(v), fake, fake, None, None) == 1
    cells, voxels = 49 * 39 * 29, 50 * 40 * 30
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), None, fake, 4, 4, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, None, 4, 4, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, -1, 4, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, -1, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, 5 * cells + 1, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 3 * voxels + 1, 4, fake, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, 4, None, fake, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, 4, fake, None, None) == 1
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 0, 0, None, None, None) == 0    # nothing to write
    v.dim[0], v.dim[1], v.dim[2] = 1 << 10, 1 << 10, 1 << 10
    assert lib.splatraster_fusion_mesh_count(C.byref(v), fake, fake, C.byref(n), None) == 4
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, 4, fake, fake, None) == 4
    v.dim[0], v.dim[1], v.dim[2] = 1, 40, 30
    assert lib.splatraster_fusion_mesh_extract(C.byref(v), fake, fake, 4, 1, fake, fake, None) == 1    # no cell: no face


def test_meshwrite_is_the_reference_s_byte_for_byte(tmp_path):
    from splatloc_amd.fusion import meshwrite
    verts, faces, norms, colors = M.write_case()
    path = tmp_path / "mesh.ply"
    meshwrite(path, verts, faces, norms, colors)
    got, want = path.read_bytes(), open(GOLDEN, "rb").read()
    assert got == want
    text = want.decode()
    assert "\n0.000001 -0.000001 2.500001 " in text and "\n-0.000000 0.000000 -0.000000 " in text    # the golden holds its edges
    assert "\n1.000000 2.000000 -3.000000 " in text and " -0.007812 " in text and len(want) < 4096
    meshwrite(path, verts[:0], faces[:0], norms[:0], colors[:0])
    assert path.read_text().endswith("property list uchar int vertex_index\nend_header\n") and "element vertex 0\n" in path.read_text()
    with pytest.raises(ValueError):
        meshwrite(path, verts, faces, norms[:5], colors)


def test_python_surface_is_present():
    import splatloc_amd.fusion as F
    assert all(hasattr(F.TSDFVolume, n) for n in ("mesh", "get_mesh", "save_mesh")) and callable(F.meshwrite)
