"""Generates the fusion fixtures by running the reference's own utils/fusion_utils.py (TSDFVolumeTorch, integrate) on the CPU, where
the reference itself pins it.  `numba` and `skimage` are stubbed: the module imports them and integrate never uses them.

The scenes are tests/fusion_reference.py's synthetic box rooms (SCENES): a camera inside an axis-aligned room, analytic z-depth,
8 poses, one frame with a block of zero depth; voxels behind the camera, outside the image and behind the walls all occur.  One
volume has 256 feature channels and margin 3, the other 8 channels and margin 2 (gen_3d_fusion_feature.py's).

Undecided voxels.  The summation order of the reference's matmul is not pinned, so a voxel whose pixel coordinate lies within
WINDOW_PX of a half-integer, whose depth_diff lies within WINDOW_M of -sdf_trunc or whose z lies within WINDOW_M of 0, in any frame
(judged on the float64 restatement), may legitimately end up elsewhere: it is stored in `undecided` and the tests skip exactly those.
Colour elements whose pre-rounding value came within WINDOW_TIE of a tie in any frame are stored in `tie`.  At most 1 % of the
voxels and 1 % of the colour elements of updated voxels may be excluded: asserted here, on the reference alone.

Bars.  Per quantity, `dev_*` = max |reference f32 - float64 restatement| over the decided voxels; the device must stay within 4 x
that of the reference's f32 result (weight: bit-exact).

Stored per scene (data only; nothing of the reference travels), each file below 1 MiB:
    grid (voxel_dim, origin, axis tables), K, poses, w2c, depth        the last three pass through BLAS / LAPACK, hence stored
    tsdf, weight [N] f32; color [N,3] u8; featsum [N] f64 (sum over the channels of the f32 feature row)
    sample_idx [S], sample_feat [S,C]                                   feature rows of a fixed sample of voxels
    undecided, tie (bit-packed), dev_tsdf, dev_color, dev_feat, dev_featsum, excluded shares, the crossing-edge count
Run: python tests/golden/make_golden_fusion.py <path of the reference checkout> (or set SPLATLOC_REFERENCE)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
SAMPLE = 192


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def generate(name, TSDFVolumeTorch, torch, R):
    cfg = R.SCENES[name]
    voxel_dim, origin = R.grid(name)
    vol = TSDFVolumeTorch(voxel_dim=torch.from_numpy(voxel_dim), origin=torch.from_numpy(origin), voxel_size=cfg["voxel_size"],
                          feat_dim=cfg["feat_dim"], margin=cfg["margin"])
    dims = [int(v) for v in vol._vol_dim]
    N, C = dims[0] * dims[1] * dims[2], cfg["feat_dim"]
    wc = vol._world_c.numpy().reshape(*dims, 4)
    axes = [wc[:, 0, 0, 0].copy(), wc[0, :, 0, 1].copy(), wc[0, 0, :, 2].copy()]
    assert np.array_equal(wc[..., :3].reshape(-1, 3), R.centres(axes)) and bool((wc[..., 3] == 1).all())

    K = R.intrinsics()
    c2w = R.poses(name).astype(np.float32)
    depth = R.analytic_depth(name, c2w.astype(np.float64))
    color_im, feat_im = R.images(name)
    w2c = np.stack([torch.inverse(torch.from_numpy(c2w[f]).float()).float().numpy() for f in range(R.FRAMES)])

    p = R.centres(axes)
    state = R.fresh_state(N, C)
    undecided, tie, updated = np.zeros(N, bool), np.zeros((N, 3), bool), np.zeros(N, bool)
    valid_share = []
    for f in range(R.FRAMES):
        vol.integrate(torch.from_numpy(depth[f]), torch.from_numpy(color_im[f]), torch.from_numpy(feat_im[f]), torch.from_numpy(K),
                      torch.from_numpy(c2w[f]))
        diag = {}
        R.integrate_f64(p, state, depth[f], color_im[f], feat_im[f], K, w2c[f], 1.0, vol.sdf_trunc, diag)
        undecided |= diag["undecided"]
        tie |= diag["tie"]
        updated |= diag["valid"]
        valid_share.append(float(diag["valid"].mean()))
    tsdf, col, wgt, feat = (t.numpy() for t in vol.get_volume())
    tsdf, wgt, col, feat = tsdf.reshape(N), wgt.reshape(N), col.reshape(N, 3), feat.reshape(N, C)
    ok = ~undecided
    assert np.array_equal(wgt[ok].astype(np.float64), state["weight"][ok]), "decided voxels must agree on who was updated"
    tie &= updated[:, None] & ok[:, None]
    share_vox = float(undecided.mean())
    share_col = float(tie.sum() / max(1, 3 * int((updated & ok).sum())))
    assert share_vox <= 0.01 and share_col <= 0.01, (share_vox, share_col)
    assert np.array_equal(col, np.rint(col)) and col.min() >= 0 and col.max() <= 255
    col_ok = ok[:, None] & ~tie
    featsum = feat.astype(np.float64).sum(axis=1)
    dev = {"dev_tsdf": np.abs(tsdf.astype(np.float64) - state["tsdf"])[ok].max(),
           "dev_color": np.abs(col.astype(np.float64) - state["color"])[col_ok].max(),
           "dev_feat": np.abs(feat.astype(np.float64) - state["feat"])[ok].max(),
           "dev_featsum": np.abs(featsum - state["feat"].sum(axis=1))[ok].max()}
    rng = np.random.default_rng(5)
    cand = np.nonzero(updated & ok)[0]
    sample = np.sort(np.concatenate([rng.choice(cand, SAMPLE - 8, replace=False), rng.choice(np.nonzero(~updated & ok)[0], 8,
                                                                                             replace=False)]))
    surf = R.surface_numpy(tsdf.reshape(dims))
    out = {"voxel_dim": voxel_dim, "origin": origin, "dims": np.array(dims, np.int64), "axis_x": axes[0], "axis_y": axes[1],
           "axis_z": axes[2], "voxel_size": np.float64(cfg["voxel_size"]), "margin": np.int64(cfg["margin"]),
           "sdf_trunc": np.float64(vol.sdf_trunc), "feat_dim": np.int64(C), "K": K, "poses": c2w, "w2c": w2c, "depth": depth,
           "tsdf": tsdf, "weight": wgt, "color": col.astype(np.uint8), "featsum": featsum, "sample_idx": sample.astype(np.int32),
           "sample_feat": feat[sample], "undecided": np.packbits(undecided), "tie": np.packbits(tie.reshape(-1)),
           "excluded": np.array([share_vox, share_col]), "valid_share": np.array(valid_share),
           "crossing_edges": np.int64(surf["verts"].shape[0]), **{k: np.float64(v) for k, v in dev.items()}}
    path = os.path.join(HERE, f"fusion_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes; dims", dims, "undecided %.3f %%, colour ties %.3f %%, valid per frame %.2f-%.2f, %d crossing edges"
          % (100 * share_vox, 100 * share_col, min(valid_share), max(valid_share), surf["verts"].shape[0]))
    print("   ", {k: float(v) for k, v in dev.items()})
    assert size < 1 << 20


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    sys.path.insert(0, ref)
    import torch
    from tests import fusion_reference as R

    stub("numba", njit=lambda *a, **k: (lambda f: f), prange=range)
    stub("skimage", measure=types.ModuleType("skimage.measure"))
    from utils.fusion_utils import TSDFVolumeTorch
    torch.set_num_threads(8)
    for name in R.SCENES:
        generate(name, TSDFVolumeTorch, torch, R)


if __name__ == "__main__":
    main()
