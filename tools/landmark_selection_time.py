"""Landmark selection timing at Replica scale on synthetic data: N = 413k key Gaussians, M = 180 views of 640 x 480 (a 221 MB
depth stack), num_gs = 5000 (test.py's default).  The scene is the synthetic room of tests/golden/make_golden_selection.py:
points near the walls and inside the room.  HIP events around each stage (inputs already on the device, one warm-up):
python tools/landmark_selection_time.py > profiles/landmark_selection_time.json"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from splatloc_amd import selection as S  # noqa: E402
from tests.golden.make_golden_selection import K, ROOM, expand_depths, look_w2c, render_mm  # noqa: E402

N, M, NUM = 413_000, 180, 5000
REPS = 3


def scene(rng):
    w2cs, mms = [], []
    for _ in range(M):
        c = np.array([rng.uniform(1.5, 6.5), rng.uniform(1.5, 4.5), rng.uniform(1.0, 2.0)])
        w2c = look_w2c(c, rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.2))
        w2cs.append(w2c)
        mms.append(render_mm(w2c, rng, 0.05))
    n_wall = N * 3 // 4
    ax = rng.integers(0, 3, n_wall)
    side = rng.integers(0, 2, n_wall)
    p = rng.uniform([0.2, 0.2, 0.2], ROOM - 0.2, size=(n_wall, 3))
    off = rng.uniform(0.0, 0.1, n_wall)
    p[np.arange(n_wall), ax] = np.where(side == 0, off, ROOM[ax] - off)
    free = rng.uniform([0.3, 0.3, 0.3], ROOM - 0.3, size=(N - n_wall, 3))
    return np.concatenate([p, free]).astype(np.float32), np.stack(w2cs), expand_depths(np.stack(mms))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


pts, w2cs, depths = scene(np.random.default_rng(0))
dp = torch.from_numpy(pts).cuda()
dw = torch.from_numpy(w2cs).cuda()
dd = torch.from_numpy(depths).cuda()
rows = []
for rep in range(REPS + 1):
    sc, t_scores, _ = timed(lambda: S.landmark_scores(dp, dw, K, dd))
    (idx, passes), t_select, w_select = timed(lambda: S.select_landmarks(dp, sc["score"], NUM, return_passes=True))
    if rep:
        rows.append({"scores_ms": round(t_scores, 3), "select_ms": round(t_select, 3), "select_wall_ms": round(w_select, 3),
                     "passes": passes})
nv = sc["n_visible"].cpu().numpy()
print(json.dumps({
    "what": f"landmark selection (HIP) on MI355X: N={N}, M={M}, num_gs={NUM}, synthetic room; HIP events per stage, "
            f"{REPS} runs after 1 warm-up; select_ms includes the input checks (isfinite, unique) and one host read per pass",
    "mean_n_visible": round(float(nv.mean()), 2),
    "visible_pairs": int(nv.sum()),
    "depth_stack_MB": round(depths.nbytes / 1e6, 1),
    "cpu_reference_extrapolated_s": round(24e-6 * N * M, 0),
    "rows": rows}, indent=1))
