"""Times superpoint.detect (csrc/superpoint_head.hip) against the same head written with torch operators on the device, as the
hloc model spends them: a softmax and a depth-to-space permute, five max-pools with their `where`s, then per image a `nonzero`
(which waits for the device), the index / border / `topk` selection and a flip, and two `normalize`s around a `grid_sample`.
480 x 640 frames (60 x 80 cells), B = 1 and 8, on two kinds of logits: "many" (more candidates than max_keypoints: the top-k
path) and "few" (fewer: the row-major path).  `dense_descriptors` gets rows of its own, with the bytes written and the fraction of
the MI355X's 8 TB/s peak HBM bandwidth they amount to.

Both sides are timed twice per sample: device events around the calls, and the host's clock from the first call to the end of a
synchronize (the torch side's host waits show in both; the HIP side has none).  The two implementations alternate in one
process, REPS rounds after a warm-up of every shape; medians and the spread per row.  Before anything is timed the outputs are
compared: the keypoint sets of every image must be equal (the order within equal scores is torch.topk's to choose).

    python tools/time_superpoint_head.py > profiles/superpoint_head_time.json
"""
import json
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from splatloc_amd import superpoint as SP  # noqa: E402

REPS = 10
INNER = 10      # calls of the HIP side per sample
HC, WC = 60, 80
RADIUS, THRESHOLD, MAX_KEYPOINTS, BORDER = 4, 0.005, 4096, 4
HBM_PEAK = 8.0e12   # bytes / s


def torch_head(semi, coarse):
    """the head with torch operators only, per image where the hloc model works per image"""
    b, _, hc, wc = semi.shape
    s = F.softmax(semi, 1)[:, :-1]
    s = s.permute(0, 2, 3, 1).reshape(b, hc, wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, hc * 8, wc * 8)
    pool = lambda x: F.max_pool2d(x, 2 * RADIUS + 1, stride=1, padding=RADIUS)   # noqa: E731
    zeros = torch.zeros_like(s)
    m = s == pool(s)
    for _ in range(2):
        supp = pool(m.float()) > 0
        q = torch.where(supp, zeros, s)
        m = m | ((q == pool(q)) & ~supp)
    s = torch.where(m, s, zeros)
    d = F.normalize(coarse, p=2, dim=1)
    out = []
    h, w = hc * 8, wc * 8
    for i in range(b):
        kp = torch.nonzero(s[i] > THRESHOLD)                 # the host waits here
        sc = s[i][kp[:, 0], kp[:, 1]]
        keep = (kp[:, 0] >= BORDER) & (kp[:, 0] < h - BORDER) & (kp[:, 1] >= BORDER) & (kp[:, 1] < w - BORDER)
        kp, sc = kp[keep], sc[keep]
        if MAX_KEYPOINTS < len(kp):
            sc, idx = torch.topk(sc, MAX_KEYPOINTS, dim=0)
            kp = kp[idx]
        kp = torch.flip(kp, [1]).float()
        g = (kp - 3.5) / torch.tensor([w - 4.5, h - 4.5], device=kp.device) * 2 - 1
        desc = F.grid_sample(d[i:i + 1], g.view(1, 1, -1, 2), mode="bilinear", align_corners=True)
        desc = F.normalize(desc.reshape(1, 256, -1), p=2, dim=1)[0]
        out.append({"keypoints": kp, "scores": sc, "descriptors": desc})
    return out


def timed(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return out, a.elapsed_time(b) / calls, wall / calls


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def inputs(kind, b, seed):
    g = torch.Generator().manual_seed(seed)
    semi = torch.randn(b, 65, HC, WC, generator=g) * 3.0
    if kind == "few":
        semi[:, 64] += 12.0
    return semi.cuda(), torch.randn(b, 256, HC, WC, generator=g).cuda()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_superpoint_head.py measures on the GPU: no HIP device is available")
    rows = []
    for kind in ("many", "few"):
        for b in (1, 8):
            semi, coarse = inputs(kind, b, 7 + b)
            hip = lambda: SP.detect(semi, coarse, RADIUS, THRESHOLD, MAX_KEYPOINTS, BORDER)   # noqa: E731
            ref = lambda: torch_head(semi, coarse)   # noqa: E731
            ours, theirs = hip(), ref()
            counts, cands = ours["count"].tolist(), ours["candidates"].tolist()
            same_sets = True
            for i in range(b):
                mine = ours["keypoints"][i, :counts[i]]
                a = set((mine[:, 1] * (8 * WC) + mine[:, 0]).long().tolist())
                t = set((theirs[i]["keypoints"][:, 1] * (8 * WC) + theirs[i]["keypoints"][:, 0]).long().tolist())
                same_sets = same_sets and a == t
            t_hip, t_ref, w_hip, w_ref = [], [], [], []
            for _ in range(REPS):
                _, ev, wall = timed(hip, INNER)
                t_hip.append(ev)
                w_hip.append(wall)
                _, ev, wall = timed(ref)
                t_ref.append(ev)
                w_ref.append(wall)
            rows.append({"what": "detect", "logits": kind, "B": b, "H": 8 * HC, "W": 8 * WC, "candidates": cands, "count": counts,
                         "keypoint_sets_equal": same_sets, "hip_device": stats(t_hip), "hip_host": stats(w_hip),
                         "torch_operators_device": stats(t_ref), "torch_operators_host": stats(w_ref)})
    for b, rows_range in ((1, None), (1, (0, 120)), (2, None)):
        _, coarse = inputs("many", b, 3)
        n_rows = 8 * HC if rows_range is None else rows_range[1] - rows_range[0]
        out = torch.empty((b, n_rows, 8 * WC, 256), dtype=torch.float32, device="cuda")
        fn = lambda: SP.dense_descriptors(coarse, rows=rows_range, out=out)   # noqa: E731
        fn()
        t_ev, t_wall = [], []
        for _ in range(REPS):
            _, ev, wall = timed(fn, INNER)
            t_ev.append(ev)
            t_wall.append(wall)
        nbytes = out.numel() * 4
        st = stats(t_ev)
        rows.append({"what": "dense_descriptors", "B": b, "rows": n_rows, "W": 8 * WC, "bytes_written": nbytes, "hip_device": st,
                     "hip_host": stats(t_wall), "write_GBps": round(nbytes / (st["median_ms"] * 1e-3) / 1e9, 1),
                     "fraction_of_hbm_peak": round(nbytes / (st["median_ms"] * 1e-3) / HBM_PEAK, 3)})
    print(json.dumps({
        "what": "superpoint.detect (HIP, one launch sequence per batch, no host wait) vs the same head with torch operators on the device "
                f"(nonzero wait included) on MI355X; {REPS} alternating rounds in one process after a warm-up; ms per call ({INNER} HIP calls "
                "per sample, one torch call); *_device: device events around the calls, *_host: host clock to the end of a synchronize; "
                f"radius {RADIUS}, threshold {THRESHOLD}, max_keypoints {MAX_KEYPOINTS}, border {BORDER}; fraction_of_hbm_peak is against "
                f"{HBM_PEAK / 1e12:.0f} TB/s",
        "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
