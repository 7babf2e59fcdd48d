"""Fused FeatureDecoder against the composed path (tinycudann.Encoding + torch layers + torch.optim.Adam) on the office_0 decoder
(32 -> 128 x 3 -> 256, 22.9 MB table): one training step at batch 256, inference at N = 5 000 and at N = 1 000 000.

HIP events, A/B interleaved in one process (region = REPS calls of one path, the two paths alternating), the median of the
regions per path and the paired ratio composed / fused per round with its min .. max as the interval.
    python tools/decoder_time.py [--rounds 8] [--out profiles/decoder_time.json]
Per-kernel times: run this script under a kernel trace with `--trace`, which runs ten fused steps and ten fused inferences only."""
import argparse
import json
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, ".")
import tinycudann as tcnn  # noqa: E402
from splatloc_amd.decoder import DecoderTrainer, FeatureDecoder, FeatureNet, _encoding_config, cos_loss  # noqa: E402

CONFIG = {"scene": {"bound": [[-3.0, 3.0], [-4.0, 2.5], [-2.0, 2.5]], "voxel_sdf": 0.06},
          "decoder": {"enc": "HashGrid", "hidden_dim": 128, "num_layers": 4, "final_dim": 256}}
FMA_PER_POINT = 32 * 128 + 128 * 128 * 2 + 128 * 256      # 69 632: one forward
F32_MATRIX_PEAK_TFLOPS = 157.0


class Composed(torch.nn.Module):
    """the parent's path: the HIP encoding module followed by torch layers"""

    def __init__(self, fused):
        super().__init__()
        self.bounding_box = fused.bounding_box.cuda()
        self.encoding = tcnn.Encoding(3, _encoding_config("HashGrid", fused.resolution_sdf), dtype=torch.float)
        d = fused.layout.dims
        self.feature_net = FeatureNet(d[0], d[1], len(d) - 1, d[-1])
        self.load_state_dict(fused.state_dict())
        self.cuda()

    def forward(self, pos):
        pos = (pos - self.bounding_box[:, 0]) / (self.bounding_box[:, 1] - self.bounding_box[:, 0])
        f = self.feature_net.model(self.encoding(pos).cuda())
        return f / f.norm(dim=-1, keepdim=True)


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def ab(fused_fn, composed_fn, rounds, reps):
    for fn in (fused_fn, composed_fn):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    f, c = [], []
    for r in range(rounds):                 # the order inside a round alternates, so drift is not charged to one path
        if r % 2 == 0:
            f.append(region(fused_fn, reps))
            c.append(region(composed_fn, reps))
        else:
            c.append(region(composed_fn, reps))
            f.append(region(fused_fn, reps))
    ratio = [y / x for x, y in zip(f, c)]
    return {"fused_ms": round(float(np.median(f)), 4), "composed_ms": round(float(np.median(c)), 4),
            "composed_over_fused_median": round(float(np.median(ratio)), 3),
            "composed_over_fused_min_max": [round(min(ratio), 3), round(max(ratio), 3)], "rounds": rounds, "calls_per_region": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    warnings.simplefilter("ignore", UserWarning)
    torch.manual_seed(0)
    fused = FeatureDecoder(CONFIG).cuda()
    with torch.no_grad():
        fused.encoding.params.uniform_(-1, 1)
    comp = Composed(fused)
    g = torch.Generator().manual_seed(1)
    lo, hi = torch.tensor(CONFIG["scene"]["bound"], dtype=torch.float64).unbind(1)

    def points(n):
        return lo + torch.rand((n, 3), generator=g, dtype=torch.float64) * (hi - lo)

    # training step at batch 256: device-resident batch for both paths (the reference hands CPU points to the module; the upload
    # is the same copy in both and is left out)
    xb = points(256).cuda()
    tb = torch.randn((256, 256), generator=g).cuda()
    trainer = DecoderTrainer(fused, lr=1e-3)
    opt = torch.optim.Adam([{"params": comp.feature_net.parameters(), "weight_decay": 1e-6, "lr": 1e-3},
                            {"params": comp.encoding.parameters(), "eps": 1e-15, "lr": 1e-3}], betas=(0.9, 0.99))

    def fused_step():
        trainer.step(xb, tb)

    def composed_step():
        loss = cos_loss(comp(xb), tb)
        opt.zero_grad()
        loss.backward()
        opt.step()

    x5k, x1m = points(5000).cuda(), points(1_000_000).cuda()

    def infer(model, x):
        def run():
            with torch.no_grad():
                model(x)
        return run

    if args.trace:
        for _ in range(10):
            fused_step()
            infer(fused, x5k)()
            infer(fused, x1m)()
        torch.cuda.synchronize()
        return
    out = {"what": "fused FeatureDecoder vs composed path (tinycudann.Encoding + torch layers + torch.optim.Adam) on MI355X, "
                   "office_0 decoder; HIP events, interleaved regions, medians",
           "train_step_batch_256": ab(fused_step, composed_step, args.rounds, 50),
           "inference_5000": ab(infer(fused, x5k), infer(comp, x5k), args.rounds, 50),
           "inference_1000000": ab(infer(fused, x1m), infer(comp, x1m), args.rounds, 5)}
    ms = out["inference_1000000"]["fused_ms"]
    out["inference_1000000"]["fused_TFLOPS"] = round(2 * FMA_PER_POINT * 1e6 / (ms * 1e-3) / 1e12, 1)
    out["inference_1000000"]["share_of_f32_matrix_peak"] = round(out["inference_1000000"]["fused_TFLOPS"] / F32_MATRIX_PEAK_TFLOPS, 3)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
