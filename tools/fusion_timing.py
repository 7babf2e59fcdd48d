"""Feature-TSDF fusion (csrc/fusion.hip) at office_0's size: 300 x 325 x 225 voxels x 256 channels (22.9 GB) and 640 x 480 x 256
synthetic frames of a box room seen from inside.  Single-frame launches and 8-frame batches against the same update composed from
torch operators on the same device (`TorchVolume`: broadcast per-axis tables, a mask, flat indices, row gathers and scatters).

HIP events; a region is one pass over the 8 frames by one path; the paths alternate inside a round and the order flips every round;
the median of the regions per path is reported, and the paired ratio with its min .. max.  Bytes touched: per valid (voxel, frame)
pair the image row (C * 4 bytes); per voxel row read and written, once per frame for single launches and once per batch for a batch;
the scalar volumes (20 bytes per voxel read, 20 per valid voxel written) are listed apart.
    python tools/fusion_timing.py [--rounds 7] [--out profiles/fusion_time.json]
    python tools/fusion_timing.py --mesh [--rounds 7] [--out profiles/fusion_mesh_time.json]
        the surface mesh (csrc/fusion_mesh.hip) on a synthetic TSDF of the same room at the same grid: surface() and the three mesh
        passes, interleaved with a device copy of 1 GiB whose rate the achieved bytes/s are set against
    python tools/fusion_timing.py --reference <checkout of the reference>     CPU only: the reference's own class on the toy volume of
                                                                              tests/golden (50 x 40 x 30 voxels, 80 x 60 x 256 frames)"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from tests.fusion_reference import look_at  # noqa: E402

BOUNDS = [[-3.0, 3.0], [-4.0, 2.5], [-2.0, 2.5]]
VOXEL, MARGIN, C, H, W, FOCAL, FRAMES = 0.02, 2, 256, 480, 640, 320.0, 8
COPY_RATE = 6.3e12     # achievable copy rate of the MI355X's HBM in bytes/s (read + write counted)


def scene(device):
    """8 poses inside the room, analytic z-depth of its walls (7 cm inside the bounds), random colour and feature images"""
    rng = np.random.default_rng(0)
    b = np.array(BOUNDS)
    K = torch.tensor([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]], dtype=torch.float32)
    poses = np.stack([look_at(b[:, 0] + (0.3 + 0.4 * rng.random(3)) * (b[:, 1] - b[:, 0]),
                              b[:, 0] + rng.random(3) * (b[:, 1] - b[:, 0])) for _ in range(FRAMES)])
    lo = torch.tensor(b[:, 0] + 0.07, device=device)
    hi = torch.tensor(b[:, 1] - 0.07, device=device)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device),
                          indexing="ij")
    rays = torch.stack([(u - K[0, 2].item()) / FOCAL, (v - K[1, 2].item()) / FOCAL, torch.ones_like(u)], dim=-1)
    depth = []
    for p in poses:
        R, eye = torch.tensor(p[:3, :3], device=device), torch.tensor(p[:3, 3], device=device)
        d = rays @ R.T
        s = torch.where(d > 0, (hi - eye) / d, torch.where(d < 0, (lo - eye) / d, torch.full_like(d, float("inf"))))
        depth.append(s.min(dim=-1).values.float())
    g = torch.Generator(device=device).manual_seed(1)
    color = torch.rand((FRAMES, H, W, 3), generator=g, device=device) * 255
    feat = torch.rand((FRAMES, H, W, C), generator=g, device=device) - 0.4
    return torch.stack(depth), color, feat, K, torch.from_numpy(poses).float()


class TorchVolume:
    """The update rule of splatraster_fusion_integrate (include/splatraster.h) composed from torch operators on the volume's own
    tensors: the camera point of every voxel by broadcasting the three per-axis tables (the kernel's summation order), a mask over
    the grid, flat voxel and pixel indices, then whole rows gathered, averaged and scattered back."""

    def __init__(self, vol):
        self.vol = vol

    def integrate(self, depth_im, color_im, feat_im, K, c2w, obs=1.0):
        vol = self.vol
        tsdf, color, weight, feat = vol.get_volume()
        tsdf, weight, color, feat = tsdf.view(-1), weight.view(-1), color.view(-1, 3), feat.view(-1, feat.shape[-1])
        ax, ay, az = vol._axis
        h, w = depth_im.shape
        m = torch.inverse(c2w.float().cpu()).tolist()
        fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
        trunc = vol.sdf_trunc

        def camera(r):      # [X, Y, Z]: ((m0 x + m1 y) + m2 z) + m3
            return ((m[r][0] * ax)[:, None, None] + (m[r][1] * ay)[None, :, None]) + (m[r][2] * az)[None, None, :] + m[r][3]

        zc = camera(2)
        u = torch.round(camera(0) * fx / zc + cx)
        v = torch.round(camera(1) * fy / zc + cy)
        seen = (zc > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        rows = seen.view(-1).nonzero().squeeze(1)
        pixel = v.view(-1)[rows].long() * w + u.view(-1)[rows].long()
        d = depth_im.reshape(-1)[pixel]
        gap = d - zc.view(-1)[rows]
        hit = (d > 0) & (gap >= -trunc)
        rows, pixel, gap = rows[hit], pixel[hit], gap[hit]
        w0 = weight[rows]
        w1 = w0 + obs
        tsdf[rows] = (w0 * tsdf[rows] + obs * torch.clamp(gap / trunc, max=1)) / w1
        weight[rows] = w1
        w0, w1 = w0[:, None], w1[:, None]
        color[rows] = ((w0 * color[rows] + obs * color_im.reshape(-1, 3)[pixel]) / w1).round().clamp(0, 255)
        feat[rows] = ((w0 * feat[rows] + obs * feat_im.reshape(-1, feat.shape[-1])[pixel]) / w1).clamp(0, 255)


def region(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def reference_cpu(ref, repeats=3):
    """the reference's TSDFVolumeTorch on this machine's CPU, at the toy size of the fixtures"""
    sys.path.insert(0, ref)
    from tests import fusion_reference as R
    for name, attrs in (("numba", dict(njit=lambda *a, **k: (lambda f: f), prange=range)),
                        ("skimage", dict(measure=types.ModuleType("skimage.measure")))):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    from utils.fusion_utils import TSDFVolumeTorch
    fx, cfg = R.fixture("c256"), R.SCENES["c256"]
    color, feat = R.images("c256")
    vol = TSDFVolumeTorch(torch.from_numpy(fx["voxel_dim"]), torch.from_numpy(fx["origin"]), cfg["voxel_size"], 256, cfg["margin"])
    args = [(torch.from_numpy(fx["depth"][f]), torch.from_numpy(color[f]), torch.from_numpy(feat[f]), torch.from_numpy(fx["K"]),
             torch.from_numpy(fx["poses"][f])) for f in range(R.FRAMES)]
    times = []
    for _ in range(repeats + 1):
        for a in args:
            t0 = time.perf_counter()
            vol.integrate(*a)
            times.append(time.perf_counter() - t0)
    times = times[R.FRAMES:]          # the first pass warms up
    # the cost follows the valid voxels: a camera outside the volume that sees all of it in free space makes every voxel valid
    full = (torch.full((R.H, R.W), 5.0), args[0][1], args[0][2], args[0][3],
            torch.from_numpy(look_at([0.0, 0.0, 2.0], [0.0, 0.0, 0.0]).astype(np.float32)))
    all_valid = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        vol.integrate(*full)
        all_valid.append(time.perf_counter() - t0)
    share = float((vol.get_volume()[2] >= repeats + 1).float().mean())      # valid in each of these frames
    return {"what": "the reference's TSDFVolumeTorch.integrate on this machine's CPU", "voxels": int(np.prod(fx["dims"])),
            "image": [R.H, R.W, 256], "threads": torch.get_num_threads(), "valid_share_per_frame": [round(float(v), 3) for v in fx["valid_share"]],
            "ms_per_frame_median": round(1e3 * float(np.median(times)), 2),
            "ms_per_frame_min_max": [round(1e3 * min(times), 2), round(1e3 * max(times), 2)],
            "free_space_frame": {"valid_share": round(share, 3), "ms_per_frame_median": round(1e3 * float(np.median(all_valid[1:])), 2)}}


def mesh_timing(rounds, out_path, inner=100):
    """surface() and the mesh passes at office_0's grid.  The TSDF is the room's own: the distance to the nearest wall (7 cm inside
    the bounds) over the truncation, clamped to [-1, 1], so the level set 0 is the six walls.  Regions: surface(0.0) as a user calls
    it (allocation, both passes, the gather of C = 256 feature rows, one host wait); splatraster_fusion_mesh_count (count kernel,
    scan, one host wait); the faces pass (memset + kernel); the normals pass; a 1 GiB device copy.  A region is `inner` calls of
    one path between two events (a single call is 0.1-0.6 ms: too short a window); milliseconds are per call.  Bytes of a pass: what it must
    read and write once (the TSDF, the offsets it uses, its output).  The TSDF (4 bytes per voxel) fits the 256 MiB Infinity Cache,
    so a pass can exceed the HBM copy rate."""
    import ctypes as Ct
    from splatloc_amd import _native
    from splatloc_amd import fusion as F
    vol = F.volume_from_bounds(BOUNDS, VOXEL, C, margin=MARGIN)
    dev = vol.device
    b = np.array(BOUNDS)
    dist = None
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = -1
        p = vol._axis[a].double()
        d = torch.minimum(p - (b[a, 0] + 0.07), (b[a, 1] - 0.07) - p).view(shape)
        dist = d if dist is None else torch.minimum(dist, d)
    vol.get_volume()[0].copy_(torch.clamp(dist / vol.sdf_trunc, -1, 1).float())
    X, Y, Z = vol.voxel_dim
    N, cells = X * Y * Z, (X - 1) * (Y - 1) * (Z - 1)
    lib, v = _native.load(), vol._native()
    nb = Ct.c_size_t(0)
    _native.check(lib.splatraster_fusion_mesh_bytes(X, Y, Z, Ct.byref(nb)), "splatraster_fusion_mesh_bytes")
    ws = torch.empty(vol.surface_bytes, dtype=torch.uint8, device=dev)
    mws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    n_v, n_f = Ct.c_int64(0), Ct.c_int64(0)
    _native.check(lib.splatraster_fusion_surface_count(Ct.byref(v), 1, 0.0, ws.data_ptr(), Ct.byref(n_v), None), "surface_count")
    _native.check(lib.splatraster_fusion_mesh_count(Ct.byref(v), ws.data_ptr(), mws.data_ptr(), Ct.byref(n_f), None), "mesh_count")
    M, Fc = int(n_v.value), int(n_f.value)
    faces = torch.empty((Fc, 3), dtype=torch.int32, device=dev)
    normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)

    def count():
        _native.check(lib.splatraster_fusion_mesh_count(Ct.byref(v), ws.data_ptr(), mws.data_ptr(), Ct.byref(n_f), None), "mesh_count")

    def extract(m, f):
        _native.check(lib.splatraster_fusion_mesh_extract(Ct.byref(v), ws.data_ptr(), mws.data_ptr(), m, f, faces.data_ptr() if f else None,
                                                          normals.data_ptr() if m else None, None), "mesh_extract")

    paths = {"surface": lambda: vol.surface(0.0), "mesh_count": count, "mesh_faces": lambda: extract(0, Fc),
             "mesh_normals": lambda: extract(M, 0), "copy_1GiB": lambda: dst.copy_(src)}
    with torch.cuda.device(dev):
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        names = list(paths)
        for r in range(rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                ms[k].append(region(lambda fn=paths[k]: [fn() for _ in range(inner)]) / inner)
    med = {k: float(np.median(t)) for k, t in ms.items()}
    copy_rate = 2 * src.numel() / (med["copy_1GiB"] * 1e-3)
    nbytes = {"mesh_count": 4 * N + 4 * cells + 8 * cells, "mesh_faces": 4 * N + 4 * cells + 12 * Fc + 12 * Fc,
              "mesh_normals": 4 * N + 4 * N + 12 * M}
    out = {"what": "surface mesh on MI355X at office_0's grid, synthetic room TSDF, level 0; HIP events, interleaved regions, medians, ms per call",
           "voxel_dim": [X, Y, Z], "voxels": N, "cells": cells, "feat_dim": C, "vertices": M, "faces": Fc, "rounds": rounds, "calls_per_region": inner,
           "ms": {k: round(t, 4) for k, t in med.items()},
           "ms_min_max": {k: [round(min(t), 4), round(max(t), 4)] for k, t in ms.items()},
           "measured_copy_TB_per_s": round(copy_rate / 1e12, 3),
           "bytes": nbytes,
           "achieved_TB_per_s": {k: round(nbytes[k] / (med[k] * 1e-3) / 1e12, 3) for k in nbytes},
           "share_of_measured_copy_rate": {k: round(nbytes[k] / (med[k] * 1e-3) / copy_rate, 3) for k in nbytes},
           "notes": "mesh_count includes the scan of the cell counts and one host wait; mesh_faces includes the memset of the faces "
                    "(counted as 12 F bytes written twice); the 4-byte TSDF (%d MB) fits the Infinity Cache" % (4 * N // 10 ** 6)}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    if args.reference:
        print(json.dumps(reference_cpu(args.reference), indent=1))
        return
    if args.mesh:
        mesh_timing(args.rounds, args.out)
        return
    from splatloc_amd import fusion as F
    vol = F.volume_from_bounds(BOUNDS, VOXEL, C, margin=MARGIN)
    dev = vol.device
    depth, color, feat, K, poses = scene(dev)
    N = int(np.prod(vol.voxel_dim))

    # valid voxels per frame, and voxels valid in at least one frame of the batch
    valid = []
    for f in range(FRAMES):
        vol.reset()
        vol.integrate(depth[f], color[f], feat[f], K, poses[f])
        valid.append(int((vol.get_volume()[2] > 0).sum()))
    vol.reset()
    vol.integrate_frames(depth, color, feat, K, poses)
    union = int((vol.get_volume()[2] > 0).sum())
    batch_volumes = [t.clone() for t in (vol.get_volume()[0], vol.get_volume()[2])]
    comp = TorchVolume(vol)
    vol.reset()
    for f in range(FRAMES):
        comp.integrate(depth[f], color[f], feat[f], K, poses[f])
    tsdf_t, _, weight_t, _ = vol.get_volume()
    agree = {"weight_equal_share": round(float((weight_t == batch_volumes[1]).double().mean()), 6),
             "tsdf_max_abs_diff_where_weights_agree": float((tsdf_t - batch_volumes[0]).abs()[weight_t == batch_volumes[1]].max())}

    def singles():
        for f in range(FRAMES):
            vol.integrate(depth[f], color[f], feat[f], K, poses[f])

    def batch():
        vol.integrate_frames(depth, color, feat, K, poses)

    def composed():
        for f in range(FRAMES):
            comp.integrate(depth[f], color[f], feat[f], K, poses[f])

    paths = {"single": singles, "batch8": batch, "torch": composed}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    names = list(paths)
    for r in range(args.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(region(paths[k]) / FRAMES)
    row = C * 4
    pairs = sum(valid)
    bytes_single = pairs * 3 * row
    bytes_batch = pairs * row + union * 2 * row
    scalars_single = FRAMES * N * 20 + pairs * 20
    scalars_batch = N * 20 + union * 20
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"what": "feature-TSDF fusion on MI355X at office_0's size; HIP events, interleaved regions of 8 frames, medians, ms per frame",
           "voxels": N, "feat_dim": C, "image": [H, W, C], "volume_bytes": vol.bytes,
           "valid_share_per_frame": [round(v / N, 4) for v in valid], "valid_in_any_frame_share": round(union / N, 4),
           "ms_per_frame": {k: round(v, 3) for k, v in med.items()},
           "ms_per_frame_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
           "torch_over_single": round(float(np.median([t / s for t, s in zip(ms["torch"], ms["single"])])), 2),
           "torch_over_batch8": round(float(np.median([t / s for t, s in zip(ms["torch"], ms["batch8"])])), 2),
           "single_over_batch8": round(float(np.median([t / s for t, s in zip(ms["single"], ms["batch8"])])), 2),
           "row_bytes_per_frame": {"single": bytes_single // FRAMES, "batch8": bytes_batch // FRAMES},
           "scalar_volume_bytes_per_frame": {"single": scalars_single // FRAMES, "batch8": scalars_batch // FRAMES},
           "achieved_TB_per_s": {"single": round((bytes_single + scalars_single) / FRAMES / (med["single"] * 1e-3) / 1e12, 3),
                                 "batch8": round((bytes_batch + scalars_batch) / FRAMES / (med["batch8"] * 1e-3) / 1e12, 3)},
           "rounds": args.rounds, "hip_vs_torch_composition": agree}
    out["share_of_copy_rate"] = {k: round(v * 1e12 / COPY_RATE, 3) for k, v in out["achieved_TB_per_s"].items()}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
