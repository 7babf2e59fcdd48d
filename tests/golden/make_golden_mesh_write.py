"""Generates tests/golden/mesh_write.ply with the reference's own meshwrite (utils/fusion_utils.py:35-76) from the seeded mesh of
tests/mesh_reference.py (write_case).  `numba` and `skimage` are stubbed as in make_golden_fusion_edges.py: the module imports them
and meshwrite never uses them.  The file is data only (an ASCII PLY of 20 vertices and 31 faces); nothing of the reference travels.

Run: python tests/golden/make_golden_mesh_write.py <path of the reference checkout> (or set SPLATLOC_REFERENCE)."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    sys.path.insert(0, ref)
    from tests import mesh_reference as M

    stub("numba", njit=lambda *a, **k: (lambda f: f), prange=range)
    stub("skimage", measure=types.ModuleType("skimage.measure"))
    from utils.fusion_utils import meshwrite
    verts, faces, norms, colors = M.write_case()
    path = os.path.join(HERE, "mesh_write.ply")
    meshwrite(path, verts, faces, norms, colors)
    text = open(path).read()
    assert "\n0.000001 -0.000001 2.500001 " in text and "\n-0.000000 0.000000 -0.000000 " in text
    assert text.count("\n") == 15 + 20 + 31
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
