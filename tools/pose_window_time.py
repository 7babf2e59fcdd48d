"""Pose refinement of 8 query frames: pose.refine_poses with window = 1, 2, 4, 5, 8 against the loop of 8 pose.refine_pose calls.

Workload: bench.py --stage pose_refine's — the S2-ref-layout scene (500k Gaussians, C = 4), 640x480, fx = fy = 572 — with 8 query
frames whose true poses differ from the start pose by about 1.5 degrees / 5 cm; and the same with a uniform cloud of 413k Gaussians
(Replica's count; NOT a reconstructed room) at a scale that gives lists of Replica's length.
Alternating regions in one process, REGIONS regions per variant of ITERS iterations for all 8 frames each (over a second), a host
clock around a device synchronise, every shape warmed first; medians and min - max per variant, in ms per frame-iteration.
Then the agreement at the sizes timed: window run vs loop, poses after 40 iterations.

python tools/pose_window_time.py [--out profiles/pose_window_time.json] [--small]
python tools/pose_window_time.py --trace W     (60 iterations at window W and nothing else: for rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from splatloc_amd import pose  # noqa: E402
from splatloc_amd.camera import PinholeCamera  # noqa: E402
from splatloc_amd.synthetic import WORKLOADS, make_scene  # noqa: E402

WINDOWS = (1, 2, 4, 5, 8)
FRAMES = 8


def setup(name, dev, small):
    from splatloc_amd import GaussianRasterizationSettings, GaussianRasterizer
    if name == "S2-ref-layout":
        wl = dict(WORKLOADS[name])
    else:
        wl = dict(P=413_000, W=640, H=480, C=4, seed=3, scale_median=0.012)
    if small:
        wl["P"] //= 50
    sc = make_scene(**wl).to(dev)
    cam = PinholeCamera(640, 480, 572.0, 572.0, 320.0, 240.0)
    cam.to(dev)
    g = torch.Generator().manual_seed(17)
    # ~1.5 degrees (0.026 rad) and ~5 cm, a different direction per frame
    w = torch.nn.functional.normalize(torch.randn(FRAMES, 3, generator=g), dim=1) * 0.026
    t = torch.nn.functional.normalize(torch.randn(FRAMES, 3, generator=g), dim=1) * 0.05
    W2C_true = pose.at_to_transform_matrix(w, t).to(dev)
    cs, ds = [], []
    with torch.no_grad():
        for M in W2C_true:
            view, proj, campos = pose.camera_tensors(M, cam.projection_matrix)
            rs = GaussianRasterizationSettings(480, 640, cam.tanfovx, cam.tanfovy, sc.bg, 1.0, view, proj, 0, campos, False, False)
            c, d, _, _ = GaussianRasterizer(raster_settings=rs)(
                means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), shs=None, colors_precomp=sc.features,
                opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations, cov3D_precomp=None)
            cs.append(c)
            ds.append(d)
    gs = dict(means3D=sc.means3D, colors=sc.features, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations)
    return sc, cam, gs, torch.stack(cs), torch.stack(ds), torch.eye(4, device=dev).repeat(FRAMES, 1, 1), int(sc.means3D.shape[0])


def measure(name, dev, regions, iters, small):
    sc, cam, gs, tc, td, W0, P = setup(name, dev, small)

    def loop(n):
        return [pose.refine_pose((tc[j], td[j]), gs, cam, W0[j], iterations=n, background=sc.bg) for j in range(FRAMES)]

    def win(w, n):
        return pose.refine_poses((tc, td), gs, cam, W0, iterations=n, background=sc.bg, window=w)

    variants = {"loop": loop, **{f"window_{w}": (lambda n, w=w: win(w, n)) for w in WINDOWS}}
    for fn in variants.values():      # every shape once
        fn(5)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in variants}
    for _ in range(regions):
        for k, fn in variants.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(iters)
            torch.cuda.synchronize(dev)
            ms[k].append(1e3 * (time.perf_counter() - t0) / (FRAMES * iters))
    # the agreement at this size: 40 iterations, window run vs loop
    ref = torch.stack([W for W, _ in loop(40)])
    agree = {f"window_{w}": float((win(w, 40)[0] - ref).abs().max()) for w in WINDOWS}
    torch.cuda.synchronize(dev)
    med = {k: statistics.median(v) for k, v in ms.items()}
    rows = {k: {"ms_per_frame_iteration": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4),
                "regions_ms": [round(x, 4) for x in v], "loop_over_this": round(med["loop"] / med[k], 3)} for k, v in ms.items()}
    spread = (max(ms["loop"]) - min(ms["loop"])) / med["loop"]
    best = min(WINDOWS, key=lambda w: med[f"window_{w}"])
    return {"workload": name, "P": P, "frames": FRAMES, "regions": regions, "iterations_per_region": iters,
            "region_seconds_loop": round(med["loop"] * FRAMES * iters / 1e3, 2), "variants": rows,
            "loop_spread_relative": round(spread, 4), "best_window": best,
            "best_beats_loop_by_more_than_its_spread": bool(med["loop"] / med[f"window_{best}"] - 1.0 > spread),
            "max_pose_difference_vs_loop_after_40_iterations": {k: float(f"{v:.3e}") for k, v in agree.items()},
            "poses_agree_within_2e-4": bool(max(agree.values()) <= 2e-4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pose_window_time.json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    ap.add_argument("--trace", type=int, default=0, metavar="W")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace:
        sc, cam, gs, tc, td, W0, _ = setup("S2-ref-layout", dev, a.small)
        pose.refine_poses((tc, td), gs, cam, W0, iterations=60, background=sc.bg, window=a.trace)
        torch.cuda.synchronize(dev)
        return
    regions, iters = (2, 10) if a.small else (7, 500)
    out = {"what": "ms per frame-iteration of pose refinement of 8 query frames at 640x480: refine_poses(window) vs the loop of "
                   "8 refine_pose calls; alternating regions in one process, host clock around a device synchronise",
           "device": torch.cuda.get_device_name(dev),
           "results": [measure(n, dev, regions, iters, a.small) for n in ("S2-ref-layout", "uniform-413k")]}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
