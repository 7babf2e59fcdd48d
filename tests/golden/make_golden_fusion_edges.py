"""Generates tests/golden/fusion_edges.npz by running the reference's own utils/fusion_utils.py (TSDFVolumeTorch, integrate) on the
CPU over the exact scenes of tests/fusion_reference.py (EDGE_SCENES), as make_golden_fusion.py does for the box rooms.  `numba` and
`skimage` are stubbed: the module imports them and integrate never uses them.

Exact scenes.  The cameras are axis-aligned (rotations of 0 and +-1 entries, dyadic translations) over dyadic grids, so every
product of the reference's matmul is exact and any summation order gives the same f32 numbers: the reference pins every voxel, the
ones exactly on a rounding edge included, and there is no `undecided` and no `tie` mask.  Asserted here, on the reference alone:
    torch.inverse of every pose is exactly the analytic inverse [R^T | -R^T t];
    the reference's axis tables are the dyadic ones the scenes state;
    the reference's four f32 volumes equal tests/fusion_reference.py's integrate_f32 bit for bit, for every scene;
    every scene reaches each of the seven kinds of tie the rounding rules have (half-integer pixel x and y, x = -0.5,
    x = W - 0.5, depth_diff == -sdf_trunc, colour means ending in .5, z == 0) at least 100 times, and the exact scenes reach
    y = -0.5 and y = H - 0.5 at least 30 times each.

Stored (data only; nothing of the reference travels), below 1 MiB: per scene the complete tsdf, weight [N] f32, color [N,3] u8 and
feat [N,C] f32 volumes, the world-to-camera matrices torch.inverse returned, and the tie counts in TIE_KINDS order followed by the
number of voxel-frames integrated.  The inputs are not stored: edge_scene() rebuilds them from integer arithmetic.
Run: python tests/golden/make_golden_fusion_edges.py <path of the reference checkout> (or set SPLATLOC_REFERENCE).  The archive
is written with fixed timestamps: the same inputs give the same bytes."""
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
SEVEN = ("px_half", "py_half", "px_low", "px_high", "diff_trunc", "color_half", "z_zero")


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def generate(name, TSDFVolumeTorch, torch, R, out):
    sc = R.edge_scene(name)
    dims, C = sc["dims"], sc["feat_dim"]
    N = dims[0] * dims[1] * dims[2]
    vol = TSDFVolumeTorch(voxel_dim=torch.tensor(dims, dtype=torch.float64), origin=torch.from_numpy(sc["origin"]),
                          voxel_size=sc["voxel_size"], feat_dim=C, margin=sc["margin"])
    wc = vol._world_c.numpy().reshape(*dims, 4)
    assert np.array_equal(wc[..., :3].reshape(-1, 3), R.centres(sc["axes"])) and bool((wc[..., 3] == 1).all())
    assert np.float32(vol.sdf_trunc if hasattr(vol, "sdf_trunc") else vol._sdf_trunc) == np.float32(sc["sdf_trunc"])
    w2c = np.stack([torch.inverse(torch.from_numpy(sc["poses"][f]).float()).float().numpy() for f in range(R.EDGE_FRAMES)])
    assert np.array_equal(w2c, sc["w2c"]), f"{name}: torch.inverse is not the analytic inverse"
    for f in range(R.EDGE_FRAMES):
        vol.integrate(torch.from_numpy(sc["depth"][f]), torch.from_numpy(sc["color"][f]), torch.from_numpy(sc["feat"][f]),
                      torch.from_numpy(sc["K"]), torch.from_numpy(sc["poses"][f]), obs_weight=sc["obs_weight"])
    tsdf, col, wgt, feat = (t.numpy() for t in vol.get_volume())
    tsdf, wgt, col, feat = tsdf.reshape(N), wgt.reshape(N), col.reshape(N, 3), feat.reshape(N, C)
    counts = {}
    state = R.integrate_scene_f32(sc, counts=counts)
    for k, got in (("tsdf", tsdf), ("weight", wgt), ("color", col), ("feat", feat)):
        assert got.dtype == np.float32 and np.array_equal(got, state[k], equal_nan=True), f"{name}: {k} differs from integrate_f32"
    assert not np.isnan(tsdf).any() and not np.isnan(feat).any()
    assert np.array_equal(col, np.rint(col)) and col.min() >= 0 and col.max() <= 255
    assert all(counts[k] >= 100 for k in SEVEN), (name, counts)
    if name in R.EXACT_SCENES:
        assert counts["py_low"] >= 30 and counts["py_high"] >= 30, (name, counts)
    out[f"{name}_tsdf"], out[f"{name}_weight"], out[f"{name}_color"], out[f"{name}_feat"] = tsdf, wgt, col.astype(np.uint8), feat
    out[f"{name}_w2c"] = w2c
    out[f"{name}_counts"] = np.array([counts[k] for k in R.TIE_KINDS] + [counts["updates"]], np.int64)
    print(name, dims, "C", C, "obs", sc["obs_weight"], {k: counts[k] for k in R.TIE_KINDS}, "updated voxels", int((wgt > 0).sum()),
          "max weight", float(wgt.max()))


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    sys.path.insert(0, ref)
    import torch
    from tests import fusion_reference as R

    stub("numba", njit=lambda *a, **k: (lambda f: f), prange=range)
    stub("skimage", measure=types.ModuleType("skimage.measure"))
    from utils.fusion_utils import TSDFVolumeTorch
    torch.set_num_threads(8)
    out = {"kinds": np.array(list(R.TIE_KINDS) + ["updates"]), "scenes": np.array(list(R.EDGE_SCENES))}
    for name in R.EDGE_SCENES:
        generate(name, TSDFVolumeTorch, torch, R, out)
    path = os.path.join(HERE, "fusion_edges.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
