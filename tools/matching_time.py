"""2D-3D matching timing on synthetic data: hungarian_solve's cost + exact assignment at SuperPoint sizes (N1 query keypoints,
N2 decoded map points, D = 256, descriptors with a correlated share like tests/golden/make_golden_matching.py), the batched
solver at B = 64, and the frustum candidates of one 640 x 480 frame against ~400k key Gaussians with ~20k keypoint pixels.
HIP events (inputs on the device, one warm-up); the CPU path (torch CPU matmul + scipy) is timed on the same host:
python tools/matching_time.py > profiles/matching_time.json"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from splatloc_amd import matching as M  # noqa: E402
from tests.golden.make_golden_matching import descriptors, look_at, ray_depth, wall_points  # noqa: E402

SIZES = [(1000, 500), (2000, 1000), (4096, 2000)]
D, REPS, BATCH = 256, 3, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def cpu_path(d1, d2):
    from scipy.optimize import linear_sum_assignment
    t0 = time.perf_counter()
    a = torch.nn.functional.normalize(torch.from_numpy(d1), p=2, dim=0)
    b = torch.nn.functional.normalize(torch.from_numpy(d2), p=2, dim=0)
    sim = a.t() @ b
    sim[sim < 0.4] = 0
    cost = 1 - sim
    t1 = time.perf_counter()
    linear_sum_assignment(cost)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


rng = np.random.default_rng(0)
rows = []
for N1, N2 in SIZES:
    d1, d2 = descriptors(rng, D, N1, N2)
    g1, g2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    lo = min(N1, N2)
    cost = torch.empty(N1 * N2, dtype=torch.float64, device="cuda")
    norms = torch.empty(N1 + N2, dtype=torch.float32, device="cuda")
    lib = M._native.load()
    from splatloc_amd.rasterizer import _stream  # noqa: E402
    st = _stream(torch.device("cuda", 0))
    full, cost_ms, solve_ms = [], [], []
    for rep in range(REPS + 1):
        (m, s, steps), t = timed(lambda: M.match_descriptors(g1, g2, return_steps=True))
        _, tc = timed(lambda: lib.splatraster_match_cost(D, N1, N2, M._ptr(g1), M._ptr(g2), 0.4, M._ptr(norms), M._ptr(cost), st))
        cm = cost.view(lo, max(N1, N2))
        _, ts = timed(lambda: M.linear_sum_assignment(cm))
        if rep:
            full.append(t)
            cost_ms.append(tc)
            solve_ms.append(ts)
    cpu = [cpu_path(d1, d2) for _ in range(2)]
    rows.append({"N1": N1, "N2": N2, "cost_plus_solve_ms": [round(x, 3) for x in full],
                 "cost_ms": [round(x, 3) for x in cost_ms], "solve_ms": [round(x, 3) for x in solve_ms],
                 "steps": steps, "steps_per_row": round(steps / lo, 3),
                 "us_per_step": round(1e3 * min(solve_ms) / steps, 3),
                 "cpu_matmul_ms": round(min(c[0] for c in cpu), 3), "cpu_scipy_ms": round(min(c[1] for c in cpu), 3)})

# batched: B problems of (1000, 500) in one call
d1, d2 = descriptors(rng, D, 1000, 500)
a = torch.nn.functional.normalize(torch.from_numpy(d1), p=2, dim=0)
b = torch.nn.functional.normalize(torch.from_numpy(d2), p=2, dim=0)
sim = a.t() @ b
sim[sim < 0.4] = 0
one = (1 - sim).double()
mats = [one.roll(k, dims=0).cuda() for k in range(BATCH)]
batch_ms = []
for rep in range(REPS + 1):
    _, t = timed(lambda: M.linear_sum_assignment_batch(mats))
    if rep:
        batch_ms.append(t)
_, t1 = timed(lambda: M.linear_sum_assignment(mats[0]))

# frustum candidates: ~400k key Gaussians, 640 x 480, ~20k keypoint pixels
W, H = 640, 480
K = np.array([[320.0, 0.0, 319.5], [0.0, 320.0, 239.5], [0.0, 0.0, 1.0]])
pts = torch.from_numpy(wall_points(rng, 400_000).astype(np.float32)).cuda()
marker = torch.from_numpy(rng.uniform(0.0, 0.02, size=400_000).astype(np.float32)).cuda()
c2w = look_at(np.array([1.5, 1.2, 1.4]), np.array([5.5, 4.0, 1.2]))
w2c = np.linalg.inv(c2w)
depth = torch.from_numpy(ray_depth(c2w, K, W, H).astype(np.float32)).cuda()
mask = torch.from_numpy((rng.random((H, W)) < 20000 / (W * H)).astype(np.int32)).cuda()
cand_ms = []
for rep in range(REPS + 1):
    (idx, _, _), t = timed(lambda: M.frustum_candidates(pts, w2c, K, W, H, marker=marker, kp_mask=mask, depth=depth,
                                                         c2w=c2w, kp_K=K))
    if rep:
        cand_ms.append(t)

print(json.dumps({
    "what": f"2D-3D matching (HIP) on MI355X, D={D}, synthetic descriptors; HIP events after 1 warm-up, {REPS} runs; "
            "cost_plus_solve_ms = match_descriptors (cost, solve, one status read, sims gather); solve_ms = linear_sum_assignment "
            "on the device cost; cpu_* = torch CPU matmul (normalise, threshold) and scipy linear_sum_assignment on the host "
            "of the same run (best of 2)",
    "rows": rows,
    "batch": {"B": BATCH, "shape": [1000, 500], "ms": [round(x, 3) for x in batch_ms], "single_ms": round(t1, 3),
              "problems_per_s": round(BATCH / (min(batch_ms) / 1e3), 1)},
    "candidates": {"points": 400_000, "keypoints": int(mask.sum()), "pairs": int(idx.numel()),
                   "ms": [round(x, 3) for x in cand_ms]}}, indent=1))
