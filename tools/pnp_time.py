"""Absolute pose timing on planted scenes (tests/test_host_pnp.py planted_scene, Replica intrinsics, 0.5 px noise): one
query of N correspondences for N in {200, 1000, 4096} and outlier shares 0.3 and 0.7, and a B = 64 batch of N = 1000 at 0.3.
HIP events around splatloc_amd.pnp.estimate_absolute_pose(_batch) (inputs on the device, one warm-up, 3 runs; the time includes
the one host read per batch of 1024 trials): python tools/pnp_time.py > profiles/pnp_time.json"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from splatloc_amd import pnp as P  # noqa: E402
from tests.test_host_pnp import REPLICA, planted_scene  # noqa: E402

REPS, BATCH = 3, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def problem(seed, n, share):
    p2, p3, _, _, _, (fx, fy, cx, cy), _ = planted_scene(seed, n, share, REPLICA)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return torch.from_numpy(p2).cuda(), torch.from_numpy(p3).cuda(), K


rows = []
for n in (200, 1000, 4096):
    for share in (0.3, 0.7):
        p2, p3, K = problem(n + int(share * 10), n, share)
        ms = []
        for rep in range(REPS + 1):
            r, t = timed(lambda: P.estimate_absolute_pose(p2, p3, K))
            if rep:
                ms.append(t)
        rows.append({"N": n, "outlier_share": share, "ms": [round(x, 3) for x in ms], "trials": int(r["trials"]),
                     "num_inliers": int(r["num_inliers"]), "success": bool(r["success"])})
probs = [problem(5000 + k, 1000, 0.3) for k in range(BATCH)]
batch_ms = []
for rep in range(REPS + 1):
    out, t = timed(lambda: P.estimate_absolute_pose_batch(probs))
    if rep:
        batch_ms.append(t)
print(json.dumps({
    "what": f"absolute pose (P3P LO-RANSAC + Cauchy LM, HIP) on MI355X, planted scenes, Replica intrinsics, 0.5 px noise; HIP "
            f"events after 1 warm-up, {REPS} runs, one host read per batch of {P.BATCH} trials included",
    "rows": rows,
    "batch": {"B": BATCH, "N": 1000, "outlier_share": 0.3, "ms": [round(x, 3) for x in batch_ms],
              "problems_per_s": round(BATCH / (min(batch_ms) / 1e3), 1),
              "all_success": all(bool(o["success"]) for o in out)}}, indent=1))
