"""One backward of a 5-view window that returns parameter AND camera gradients, three ways on the same frame:

  joint       rasterizer.window_backward(cameras=True)  (splatraster_backward_window_joint: one compositing backward)
  two_calls   rasterizer.window_backward, then rasterizer.window_backward_cameras  (what there was before: two compositing backwards)
  per_view    five rasterizer.view_backward(want_pose=True) calls on five per-view frames

Workloads: SplatLoc's layout (640x480, C = 4, a uniform cloud of 413k Gaussians — Replica's count, NOT a reconstructed room) and
S2 (1920x1080, C = 35, 500k).  The forwards run once, outside the clock; only backwards are timed.  Alternating regions in one
process, 7 regions per variant of 1000 (200 at S2) backwards each — a second and more —, a host clock around a device synchronise, every variant warmed
first; medians and min - max per variant, in ms per backward of the window.  Then the agreement of the three at the sizes timed.

python tools/joint_window_time.py [--out profiles/joint_window_time.json] [--small]"""
import argparse
import json
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from splatloc_amd import GaussianRasterizationSettings  # noqa: E402
from splatloc_amd import rasterizer as R  # noqa: E402
from splatloc_amd.camera import PinholeCamera  # noqa: E402
from splatloc_amd.synthetic import WORKLOADS, make_scene  # noqa: E402

VIEWS = 5


def setup(name, dev, small):
    wl = dict(WORKLOADS["S2"]) if name == "S2" else dict(P=413_000, W=640, H=480, C=4, seed=3, scale_median=0.012)
    if small:
        wl["P"] //= 50
    sc = make_scene(**wl).to(dev)
    W, H, Cn = wl["W"], wl["H"], wl["C"]
    cam0 = sc.camera
    g = torch.Generator().manual_seed(23)
    settings, grads = [], []
    for k in range(VIEWS):      # five cameras around the scene's own: a few hundredths of a radian and a few centimetres apart
        ang = 0.03 * (k - VIEWS // 2)
        Rm = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]], dtype=torch.float32)
        cam = PinholeCamera(W, H, cam0.fx, cam0.fy, cam0.cx, cam0.cy, Rm, torch.tensor([0.02 * k, -0.01 * k, 0.05 * k])).to(dev)
        settings.append(GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, sc.bg, 1.0, cam.world_view_transform,
                                                      cam.full_proj_transform, 0, cam.camera_center, False, False))
        grads.append(tuple(((2.0 * torch.rand(c, H, W, generator=g) - 1.0) / (H * W)).to(dev) for c in (Cn, 1, 1)))
    return sc, settings, grads, int(sc.means3D.shape[0])


def measure(name, dev, regions, iters, small):
    sc, settings, grads, P = setup(name, dev, small)
    lib = R._native.load()
    with torch.no_grad():
        fw = R.window_forward(sc.means3D, sc.features, sc.opacities, sc.scales, sc.rotations, None, settings)
        f1 = [R.view_forward(sc.means3D, None, sc.features, sc.opacities, sc.scales, sc.rotations, None, rs) for rs in settings]
    ws = torch.empty((lib.splatraster_window_camera_workspace_bytes(VIEWS),), dtype=torch.uint8, device=dev)
    g4 = [(gc, None, gd, ga) for gc, gd, ga in grads]

    def joint():
        return R.window_backward(fw, g4, cameras=True, workspace=ws)

    def two_calls():
        d = R.window_backward(fw, g4)
        d.update(R.window_backward_cameras(fw, grads, ws))
        return d

    def per_view():
        return [R.view_backward(f, *gs, want_pose=True) for f, gs in zip(f1, grads)]

    variants = {"joint": joint, "two_calls": two_calls, "per_view": per_view}
    with torch.no_grad():
        for fn in variants.values():      # every variant once
            fn()
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in variants}
        for _ in range(regions):
            for k, fn in variants.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _i in range(iters):
                    fn()
                torch.cuda.synchronize(dev)
                ms[k].append(1e3 * (time.perf_counter() - t0) / iters)
        # the agreement at this size (float-atomic sums in different orders)
        a, b, c = joint(), two_calls(), per_view()
        torch.cuda.synchronize(dev)

    def rel(x, y):
        return float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
    agree = {"view_vs_two_calls": rel(a["view"], b["view"]), "proj_vs_two_calls": rel(a["proj"], b["proj"]),
             "means3D_vs_two_calls": rel(a["m3"], b["m3"]), "colors_vs_two_calls": rel(a["col"], b["col"]),
             "view_vs_per_view": rel(a["view"], torch.stack([d["view"] for d in c])),
             "means3D_vs_per_view": rel(a["m3"], sum(d["m3"] for d in c))}
    med = {k: statistics.median(v) for k, v in ms.items()}
    rows = {k: {"ms_per_window_backward": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4),
                "regions_ms": [round(x, 4) for x in v], "this_over_joint": round(med[k] / med["joint"], 3)} for k, v in ms.items()}
    spread = (max(ms["joint"]) - min(ms["joint"])) / med["joint"]
    return {"workload": name, "P": P, "width": settings[0].image_width, "height": settings[0].image_height,
            "channels": int(sc.features.shape[1]), "views": VIEWS, "instances_per_view": fw.R, "regions": regions,
            "backwards_per_region": iters, "variants": rows, "joint_spread_relative": round(spread, 4),
            "joint_beats_two_calls_by_more_than_its_spread": bool(med["two_calls"] / med["joint"] - 1.0 > spread),
            "max_difference_relative_to_max": {k: float(f"{v:.3e}") for k, v in agree.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/joint_window_time.json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    regions = 5 if a.small else 7
    iters = {"splatloc-layout-413k": 3 if a.small else 1000, "S2": 3 if a.small else 200}    # regions of about a second and more
    out = {"what": "ms per backward of a 5-view window that returns parameter and camera gradients: the joint call vs "
                   "window_backward + window_backward_cameras vs five per-view calls; the same frame, alternating regions in one "
                   "process, host clock around a device synchronise, forwards outside the clock",
           "device": torch.cuda.get_device_name(dev),
           "results": [measure(n, dev, regions, iters[n], a.small) for n in ("splatloc-layout-413k", "S2")]}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
