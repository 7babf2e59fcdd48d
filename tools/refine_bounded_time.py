#!/usr/bin/env python3
"""Does the bounded refinement loop queue ahead?  `training.refine_bounded` against THIS TREE's loop of `color_refinement_step`
calls on the same model, the same cameras and the same device, in ONE process, interleaved (tools/ab.py's rule: only same-box,
alternating, paired regions resolve a small effect).  The plain loop is this tree's, not a build of the parent commit: the bounded
loop needs this tree's library, and one process loads one library; the plain path's Python and its kernel instantiations are the
parent's unchanged.

Per shape: `rounds` rounds, each one region of N iterations of either loop, in an order that alternates from round to round; a
region ends in a device synchronise and its wall time is a host clock around it.  Reported per loop: wall us per iteration (every
region, their median), host enqueue us per iteration (the host clock up to the last enqueue, before the final wait), and — from a
separate, profiled region, because tracing slows the host — the summed kernel time per iteration (torch.profiler device time
stamps of every kernel in the process).  Per shape: the paired differences plain - bounded per round, their mean and their
spread; the bounded loop counts as faster when the mean exceeds the paired spread (2 standard errors).
Shapes: S0, the reference layout (640x480, C = 4) at 413k and at 500k Gaussians.
usage: python tools/refine_bounded_time.py [--shapes S0,ref-413k,ref-500k] [--iterations 300] [--rounds 6] [--out profiles/refine_bounded_time.json]"""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {"S0": dict(P=10_000, W=640, H=480, C=3, seed=0, scale_median=0.02),
          "ref-413k": dict(P=413_000, W=640, H=480, C=4, seed=2, scale_median=0.00627),
          "ref-500k": dict(P=500_000, W=640, H=480, C=4, seed=2, scale_median=0.00627)}


def build(shape, dev):
    """the model and the eight cameras of tools/refine_idle.py"""
    from splatloc_amd.camera import PinholeCamera
    from splatloc_amd.optim import Adam as FusedAdam
    from splatloc_amd.synthetic import make_scene
    wl = SHAPES[shape]
    sc = make_scene(**wl)
    P0, W, H, C = wl["P"], wl["W"], wl["H"], wl["C"]
    E = max(C - 3, 1)
    g = torch.Generator().manual_seed(11)
    par = lambda t: torch.nn.Parameter(t.to(dev).contiguous().requires_grad_(True))  # noqa: E731
    names = ("xyz", "f_dc", "f_rest", "opacity", "marker", "kp_score", "scaling", "rotation")
    attr = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "marker": "_marker",
            "kp_score": "_kp_score", "scaling": "_scaling", "rotation": "_rotation"}
    lr = {"xyz": 1.6e-4 * 6.0, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 5e-2, "marker": 5e-2, "kp_score": 5e-2,
          "scaling": 1e-3 * 6.0, "rotation": 1e-3}
    pc = types.SimpleNamespace(
        _xyz=par(sc.means3D.clone()), _features_dc=par(((sc.features[:, :3] - 0.5) / 0.28209479177387814)[:, None, :].contiguous()),
        _features_rest=par(torch.zeros(P0, 0, 3)), _opacity=par(torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))),
        _marker=par((torch.rand(P0, 1, generator=g) < 0.05).float() * torch.rand(P0, 1, generator=g) * 0.9),
        _kp_score=par(torch.rand(P0, E, generator=g)), _scaling=par(torch.log(sc.scales)), _rotation=par(sc.rotations.clone()),
        active_sh_degree=0, max_sh_degree=0, lr_init=1.6e-4 * 6.0, lr_final=1.6e-6 * 6.0, lr_delay_mult=0.01, max_steps=30000)
    pc.optimizer = FusedAdam([{"params": [getattr(pc, attr[k])], "lr": lr[k], "name": k} for k in names], lr=0.0, eps=1e-15)
    pc.max_radii2D = torch.zeros(P0, device=dev)
    views = []
    for k in range(8):
        ang = torch.tensor(0.02 * (k - 4))
        R = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]])
        cam = PinholeCamera(W, H, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, R, torch.tensor([0.01 * k, 0.0, 0.0])).to(dev)
        cam.original_image = torch.rand(3, H, W, generator=g).to(dev)
        views.append(cam)
    return pc, views


def kernel_us(run, n, dev):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run(n)
        torch.cuda.synchronize(dev)
    total, launches = 0.0, 0
    for e in prof.key_averages():
        dt = getattr(e, "device_time_total", None)
        if dt is None:
            dt = getattr(e, "cuda_time_total", 0)
        if dt and e.count:
            total += dt
            launches += e.count
    return total / n, launches / n


def measure(shape, N, rounds, dev):
    from splatloc_amd.training import color_refinement_step, refine_bounded
    pc, views = build(shape, dev)
    pipe = types.SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False)
    bg = torch.zeros(3, device=dev)
    it = [0]
    info = {"rewinds": 0, "capacity": None, "bounded": None}

    def cams(n):      # the same cycle through the eight views for both loops
        return [views[(it[0] + 1 + i) % 8] for i in range(n)]

    def plain(n):
        t0 = time.perf_counter()
        for cam in cams(n):
            it[0] += 1
            color_refinement_step(cam, pc, pipe, bg, 0.2, it[0])
        return time.perf_counter() - t0

    def bounded(n):
        res = refine_bounded(cams(n), pc, pipe, bg, 0.2, it[0] + 1, n, initial_capacity=info["capacity"])
        it[0] += n
        info["rewinds"] += res["rewinds"]
        info["bounded"] = res["bounded"]
        info["capacity"] = res["capacity_history"][-1] if res["capacity_history"] else None
        return res["enqueue_seconds"]

    loops = {"plain": plain, "bounded": bounded}
    for fn in loops.values():           # warm every shape both loops use
        fn(40)
    torch.cuda.synchronize(dev)
    info["rewinds"] = 0
    wall = {k: [] for k in loops}
    host = {k: [] for k in loops}
    for r in range(rounds):
        for k in (("plain", "bounded") if r % 2 == 0 else ("bounded", "plain")):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            enq = loops[k](N)
            torch.cuda.synchronize(dev)
            wall[k].append((time.perf_counter() - t0) / N * 1e6)
            host[k].append(enq / N * 1e6)
    out = {"shape": shape, **SHAPES[shape], "iterations_per_region": N, "rounds": rounds, "bounded_mode_ran": info["bounded"],
           "rewinds_in_timed_regions": info["rewinds"], "capacity": info["capacity"]}
    for k in loops:
        kus, launches = kernel_us(loops[k], 60, dev)
        w = sorted(wall[k])
        out[k] = {"wall_us_per_iteration": round(w[len(w) // 2], 1), "wall_us_all_regions": [round(x, 1) for x in wall[k]],
                  "host_enqueue_us_per_iteration": round(sorted(host[k])[len(host[k]) // 2], 1),
                  "kernel_us_per_iteration_torch_profiler": round(kus, 1), "kernels_per_iteration": round(launches, 1)}
    d = [a - b for a, b in zip(wall["plain"], wall["bounded"])]
    mean = sum(d) / len(d)
    sd = math.sqrt(sum((x - mean) ** 2 for x in d) / (len(d) - 1)) if len(d) > 1 else float("nan")
    spread = 2.0 * sd / math.sqrt(len(d)) if len(d) > 1 else float("nan")
    out["paired_plain_minus_bounded_us"] = {"per_round": [round(x, 1) for x in d], "mean": round(mean, 1), "sd": round(sd, 1),
                                            "two_standard_errors": round(spread, 1)}
    out["bounded_faster_beyond_paired_spread"] = bool(mean > spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="S0,ref-413k,ref-500k")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bounded_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_bounded_time: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/refine_bounded_time.py", "device": torch.cuda.get_device_name(dev),
           "what": "refine_bounded vs this tree's plain loop of color_refinement_step calls (not a build of the parent commit), "
                   "interleaved regions in one process",
           "not_measured": "why the bounded loop's summed kernel time differs from the plain loop's",
           "shapes": [measure(s, a.iterations, a.rounds, dev) for s in a.shapes.split(",")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
