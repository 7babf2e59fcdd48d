"""Host side of the tinycudann drop-in: the grid-encoding level table (splatraster_grid_encoding_layout) against an independent
Python restatement of its formula, configuration errors, and an import that opens no device.  No GPU needed."""
import ctypes
import ctypes.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (scene, bound, voxel_sdf) of SplatLoc's configs/replica_nerf/*.yaml and configs/scenes12/*.yaml
SCENES = [
    ("office_0", [[-3, 3], [-4, 2.5], [-2, 2.5]], 0.06),
    ("office_1", [[-2, 3.2], [-1.7, 2.7], [-1.2, 2.0]], 0.06),
    ("office_2", [[-3.6, 3.2], [-3.0, 5.5], [-1.4, 1.7]], 0.06),
    ("office_3", [[-5.3, 3.7], [-6.1, 3.4], [-1.4, 2.0]], 0.06),
    ("office_4", [[-1.4, 5.5], [-2.5, 4.4], [-1.4, 1.8]], 0.06),
    ("room_0", [[-1.0, 7.0], [-1.3, 3.7], [-1.7, 1.4]], 0.06),
    ("room_1", [[-5.6, 1.4], [-3.2, 2.8], [-1.6, 1.8]], 0.06),
    ("room_2", [[-1.0, 6.1], [-3.4, 1.9], [-3.1, 0.8]], 0.06),
    ("apt1_kitchen", [[-3.6, 0.1], [-4.1, 0.7], [-0.2, 2.2]], 0.06),
    ("apt1_living", [[-4.0, 2.0], [-0.4, 3.2], [0.0, 1.5]], 0.06),
    ("apt2_bed", [[-1.4, 2.4], [-5.9, -2.2], [-0.1, 1.3]], 0.06),
    ("apt2_kitchen", [[-1.6, 2.2], [-1.6, 1.5], [-0.1, 2.1]], 0.06),
    ("apt2_living", [[-2.5, 2.5], [-2.7, 2.8], [-0.3, 1.7]], 0.06),
    ("apt2_luke", [[-2.4, 2.7], [-1.8, 5.9], [-0.2, 2.6]], 0.06),
    ("of1_gates362", [[-8.8, -4.0], [-2.4, 0.8], [-0.5, 2.7]], 0.06),
    ("of1_gates381", [[2.9, 7.0], [-0.3, 5.4], [-0.6, 1.7]], 0.06),
    ("of1_lounge", [[-3.7, 3.0], [-1.9, 2.3], [-0.1, 2.1]], 0.06),
    ("of1_manolis", [[-2.5, 2.3], [-3.3, 2.5], [-0.1, 2.8]], 0.06),
    ("of2_5a", [[-4.5, 3.5], [5.4, 8.8], [-0.2, 1.3]], 0.06),
    ("of2_5b", [[-1.4, 2.9], [-5.6, 5.2], [-0.2, 2.0]], 0.06),
]


def desired_resolution(bound, voxel):
    """FeatureDecoder.resolution_sdf: int(max extent / voxel_sdf), in float64 (numpy bounds)"""
    b = np.array(bound, dtype=np.float64)
    return int((b[:, 1] - b[:, 0]).max() / voxel)


def splatloc_config(desired, otype="HashGrid"):
    """models/encoding.py's hash-grid configuration for a desired finest resolution"""
    return {"otype": otype, "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
            "per_level_scale": float(np.exp2(np.log2(desired / 16) / 15))}


_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.log2f.restype = _libm.exp2f.restype = ctypes.c_float
_libm.log2f.argtypes = _libm.exp2f.argtypes = [ctypes.c_float]
f32 = np.float32


def restated_layout(D, L, F, log2_T, base, pls, kind):
    """the level table, restated from the formula (f32 steps rounded one at a time)"""
    log2_b = f32(_libm.log2f(f32(pls)))
    levels, offset = [], 0
    for lvl in range(L):
        scale = f32(f32(_libm.exp2f(f32(f32(lvl) * log2_b))) * f32(base)) - f32(1)
        res = int(math.ceil(float(scale))) + 1
        dense = min(res ** D, 2 ** 31 - 1)
        size = (dense + 7) // 8 * 8
        if kind == "hash":
            size = min(size, 2 ** log2_T)
        elif kind == "tiled":
            size = min(size, base ** D)
        levels.append(dict(offset=offset, size=size, res=res, scale=float(scale), hashed=kind == "hash" and res ** D > size))
        offset += size
    return levels, F * offset


def _check(lay, D, L, F, log2_T, base, pls, kind):
    levels, n_params = restated_layout(D, L, F, log2_T, base, pls, kind)
    assert lay.n_params == n_params
    assert lay.offsets == [lv["offset"] for lv in levels]
    assert lay.sizes == [lv["size"] for lv in levels]
    assert lay.resolutions == [lv["res"] for lv in levels]
    assert lay.scales == [lv["scale"] for lv in levels]      # bit-identical f32 values
    assert lay.n_output_dims == L * F
    return levels


@pytest.mark.parametrize("scene,bound,voxel", SCENES, ids=[s[0] for s in SCENES])
def test_layout_of_every_splatloc_scene(scene, bound, voxel):
    from splatloc_amd.grid_encoding import GridLayout
    cfg = splatloc_config(desired_resolution(bound, voxel))
    _check(GridLayout(3, cfg), 3, 16, 2, 19, 16, cfg["per_level_scale"], "hash")


# scene: (desired resolution, res_0, res_15, dense-indexed levels, n_params).  res_15 of office_0 is 108 with a correctly rounded
# log2f (log2_b = 0.18365915f, scale_15 = 106.999985f); a log2f one ulp higher (0.18365917f) would make it 109.
TABLE = {"office_0": (108, 16, 108, 13, 5_724_048), "office_1": (86, 16, 86, 15, 4_281_952),
         "apt2_bed": (63, 16, 64, 16, 2_135_184)}


@pytest.mark.parametrize("scene", sorted(TABLE))
def test_layout_table_rows(scene):
    from splatloc_amd.grid_encoding import GridLayout
    bound, voxel = next((b, v) for s, b, v in SCENES if s == scene)
    desired, r0, r15, n_dense, n_params = TABLE[scene]
    assert desired_resolution(bound, voxel) == desired
    lay = GridLayout(3, splatloc_config(desired))
    assert lay.resolutions[0] == r0 and lay.resolutions[-1] == r15
    assert sum(r ** 3 <= s for r, s in zip(lay.resolutions, lay.sizes)) == n_dense
    assert lay.n_params == n_params


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind,otype", [("hash", {"otype": "HashGrid"}), ("dense", {"otype": "DenseGrid"}),
                                        ("tiled", {"otype": "TiledGrid"}), ("hash", {"otype": "Grid", "type": "Hash"}),
                                        ("dense", {"otype": "grid", "type": "dense"}), ("tiled", {"otype": "Grid", "type": "Tiled"})])
@pytest.mark.parametrize("L,F,log2_T,base,pls", [(16, 2, 19, 16, 1.38), (4, 2, 19, 16, 2.0), (8, 4, 14, 4, 1.5),
                                                 (32, 1, 12, 2, 1.26), (3, 8, 10, 5, 1.7)])
def test_layout_all_grid_types(D, kind, otype, L, F, log2_T, base, pls):
    from splatloc_amd.grid_encoding import GridLayout
    cfg = dict(otype, n_levels=L, n_features_per_level=F, log2_hashmap_size=log2_T, base_resolution=base,
               per_level_scale=pls, interpolation="Linear")
    levels, n_params = restated_layout(D, L, F, log2_T, base, pls, kind)
    if n_params // F > 2 ** 31 - 1:           # beyond the table the kernels index (dense grids of fine levels)
        with pytest.raises(ValueError, match="2\\^31 table entries"):
            GridLayout(D, cfg)
        return
    lay = GridLayout(D, cfg)
    levels = _check(lay, D, L, F, log2_T, base, pls, kind)
    assert lay.n_input_dims == D and lay.n_output_dims == L * F
    if kind == "dense":
        assert all(lv["size"] >= lv["res"] ** D for lv in levels)


def test_defaults_follow_tiny_cuda_nn():
    from splatloc_amd.grid_encoding import GridLayout
    lay = GridLayout(3, {"otype": "HashGrid"})      # n_levels 16, F 2, log2_T 19, base 16, per_level_scale 2
    _check(lay, 3, 16, 2, 19, 16, 2.0, "hash")
    assert lay.n_output_dims == 32


@pytest.mark.parametrize("D,cfg", [
    (3, {"otype": "SphericalHarmonics", "degree": 4}),
    (3, {"otype": "OneBlob", "n_bins": 16}),
    (3, {"otype": "Frequency", "n_frequencies": 12}),
    (3, {"otype": "Identity"}),
    (3, {"otype": "HashGrid", "interpolation": "Nearest"}),
    (3, {"otype": "HashGrid", "interpolation": "Smoothstep"}),
    (3, {"otype": "Grid", "type": "Octree"}),
    (4, {"otype": "HashGrid"}),
    (1, {"otype": "HashGrid"}),
    (3, {"otype": "HashGrid", "n_features_per_level": 3}),
    (3, {"otype": "HashGrid", "n_levels": 33}),
    (3, {"otype": "HashGrid", "n_levels": 0}),
    (3, {"otype": "HashGrid", "log2_hashmap_size": 31}),
    (3, {"otype": "HashGrid", "per_level_scale": -1.0}),
    (3, {"otype": "HashGrid", "base_resolution": 0}),
    (3, {"otype": "DenseGrid", "n_levels": 8, "per_level_scale": 4.0}),     # 2^31 table entries and more
])
def test_unsupported_configs_raise_value_error(D, cfg):
    from splatloc_amd.grid_encoding import GridLayout
    with pytest.raises(ValueError, match="supported"):
        GridLayout(D, cfg)


def test_half_precision_raises_value_error():
    import torch
    import tinycudann as tcnn
    with pytest.raises(ValueError, match="supported"):
        tcnn.Encoding(3, {"otype": "HashGrid"}, dtype=torch.half)
    with pytest.raises(ValueError, match="supported"):
        tcnn.Encoding(3, {"otype": "Frequency"}, dtype=torch.float)


def test_layout_call_rejects_bad_arguments():
    from splatloc_amd import _native
    lib = _native.load()
    lay = _native.GridLayout()
    assert lib.splatraster_grid_encoding_layout(3, 16, 2, 19, 16, 1.38, 0, None) == 1
    assert lib.splatraster_grid_encoding_layout(3, 16, 2, 19, 16, 1.38, 7, ctypes.byref(lay)) == 3
    assert lib.splatraster_grid_encoding_layout(3, 16, 2, 19, 16, float("nan"), 0, ctypes.byref(lay)) == 1
    assert lib.splatraster_grid_encoding_layout(3, 16, 2, 19, 16, 1.38, 0, ctypes.byref(lay)) == 0
    # the kernels re-validate a layout before indexing with it
    lay.offset[3] += 8
    assert lib.splatraster_grid_encoding_forward(ctypes.byref(lay), 1, None, None, None, None) == 1


def test_import_opens_no_device():
    code = ("import torch, tinycudann, simple_knn._C, diff_gauss; "
            "from tinycudann import Encoding; "
            "assert not torch.cuda.is_initialized(); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
