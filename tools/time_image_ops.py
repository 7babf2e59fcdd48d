"""Times image_ops.compute_grad_masks (csrc/image_ops.hip) against a torch-operator restatement of Camera.compute_grad_mask
(utils/camera_utils.py:145-172: the Scharr and validity convolutions, then for "replica" the Python loop over 32 x 32 blocks with one
median() and two boolean-indexed writes each) at 640 x 480 and 1200 x 680, both dataset types, N = 1 and N = 8 frames.  The torch side
handles a frame per call, as the reference does, so its time for N frames is N calls.

Device events around each sample (one call of the torch side, INNER back-to-back calls of the HIP side, per call), the two implementations alternating in one process (REPS rounds after a warm-up of every shape), frames
already on the device; medians and the spread (min, max) per row.  The outputs are compared before anything is timed: the decided 0 / 1
region must agree except where torch's own convolution rounding moves a pixel across its threshold (counted and reported).

    python tools/time_image_ops.py > profiles/image_ops_time.json
"""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from splatloc_amd import image_ops  # noqa: E402
from tests import image_ops_reference as R  # noqa: E402

REPS = 10
INNER = 20      # calls of the HIP side per sample (a call is tens of microseconds)
SHAPES = ((480, 640), (680, 1200))
EDGE_THRESHOLD = 4.0


SCHARR_V = ((3.0, 10.0, 3.0), (0.0, 0.0, 0.0), (-3.0, -10.0, -3.0))
SCHARR_H = tuple(zip(*SCHARR_V))


def _conv3(plane, weights):
    """[1,H+2,W+2] padded plane * a 3 x 3 kernel -> [1,H,W] (one conv2d launch, as the reference spends per output)"""
    k = torch.tensor(weights, dtype=torch.float32, device=plane.device).view(1, 1, 3, 3)
    return torch.nn.functional.conv2d(plane[None], k)[0]


def torch_grad_mask(image, edge_threshold, dataset_type, eps=0.01):
    """One frame with torch operators only, operator for operator what Camera.compute_grad_mask spends: a mean, a reflect pad and two
    convolutions for the gradients, a pad and two convolutions for the validity masks, the intensity, then for "replica" a Python loop
    over the 32 x 32 blocks with one median() and two boolean-indexed in-place writes per block (each index operation synchronises with
    the host), else one median() over the frame."""
    gray = image.mean(dim=0, keepdim=True)
    padded = torch.nn.functional.pad(gray, (1, 1, 1, 1), mode="reflect")
    grad_v = _conv3(padded, SCHARR_V) / 32.0
    grad_h = _conv3(padded, SCHARR_H) / 32.0
    big = (torch.nn.functional.pad(gray, (1, 1, 1, 1), mode="reflect").abs() > eps).float()
    ones = ((1.0,) * 3,) * 3
    valid_v = _conv3(big, ones) == 9.0
    valid_h = _conv3(big, ones) == 9.0
    x = torch.sqrt((grad_v * valid_v) ** 2 + (grad_h * valid_h) ** 2)
    if dataset_type != "replica":
        return x > x.median() * edge_threshold
    _, h, w = image.shape
    bh, bw = h // 32, w // 32
    for r in range(32):
        for c in range(32):
            block = x[:, r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
            t = block.median() * edge_threshold
            block[block > t] = 1
            block[block <= t] = 0
    return x


def timed(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b) / calls


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_image_ops.py measures on the GPU: no HIP device is available")
    rows = []
    for H, W in SHAPES:
        frames = torch.from_numpy(np.stack([R.frame(H, W, 100 + i) for i in range(8)])).cuda()
        for dataset_type in ("replica", "12scenes"):
            for N in (1, 8):
                batch = frames[:N].contiguous()
                hip = lambda: image_ops.compute_grad_masks(batch, EDGE_THRESHOLD, dataset_type)   # noqa: E731
                ref = lambda: [torch_grad_mask(batch[i], EDGE_THRESHOLD, dataset_type) for i in range(N)]   # noqa: E731
                ours, theirs = hip(), ref()                      # warm-up of both, and the comparison
                differ = sum(int(((ours[i] != 0) != (theirs[i] != 0)).sum()) for i in range(N))
                t_hip, t_ref = [], []
                for _ in range(REPS):
                    t_hip.append(timed(hip, INNER)[1])
                    t_ref.append(timed(ref)[1])
                row = {"H": H, "W": W, "dataset_type": dataset_type, "N": N, "path": image_ops.path(H, W) if dataset_type == "replica" else None,
                       "hip": stats(t_hip), "torch_operators": stats(t_ref), "pixels_that_differ": differ}
                row["ratio_of_medians"] = round(row["torch_operators"]["median_ms"] / row["hip"]["median_ms"], 1)
                rows.append(row)
    print(json.dumps({
        "what": "compute_grad_masks (HIP, one launch sequence for N frames) vs the torch-operator restatement of Camera.compute_grad_mask "
                f"(N calls) on MI355X; device events, alternating in one process, {REPS} rounds after a warm-up, ms per call ({INNER} HIP calls per sample); edge_threshold "
                f"{EDGE_THRESHOLD}; pixels_that_differ counts 0 / 1 disagreements (convolution rounding at a threshold, raw remainder values)",
        "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
