"""Times the convolution backbones (splatloc_amd/convnet.py, csrc/conv2d.hip) at 480 x 640 for B = 1 and B = 8: every distinct layer
shape of SuperPoint's encoder and heads and of NetVLAD's VGG16 trunk, and the two whole networks, against
torch.nn.functional.conv2d (+ relu, + max_pool2d) in float32 on the same device and against the layer's MFMA floor
2 * k * k * Cin * Cout * H * W * B / 157.3e12 (the exact-f32 MFMA peak of the MI355X; the floor is not that peak halved).

The implementations alternate in one process, REPS rounds after a warm-up of every shape; device events around INNER calls per
sample; medians and the spread per row.  Before anything is timed the outputs are compared.

    python tools/time_convnet.py > profiles/convnet_time.json
"""
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from splatloc_amd import convnet as CN  # noqa: E402

REPS = 10
INNER = 3
H0, W0 = 480, 640
PEAK = 157.3e12   # f32 MFMA, FLOP / s


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(fns):
    for fn in fns.values():      # warm-up of every shape (and the library's kernel choice)
        fn()
        fn()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn, INNER))
    return {k: stats(v) for k, v in ms.items()}


def torch_layer(x, w, b, relu, pool):
    y = F.conv2d(x, w, b, padding=(w.shape[2] - 1) // 2)
    if relu:
        y = F.relu(y)
    return F.max_pool2d(y, 2) if pool else y


def superpoint_layers():
    """(name, Cin, Cout, H, W, k, relu, pool) down the encoder and both heads"""
    res, h, w = [], H0, W0
    for name, pool in CN.SUPERPOINT_ENCODER:
        cin, cout = CN.SUPERPOINT_WIDTHS[name]
        res.append((name, cin, cout, h, w, 3, True, pool))
        h, w = CN.out_size(h, w, pool)
    for name in ("convPa", "convPb", "convDa", "convDb"):
        cin, cout = CN.SUPERPOINT_WIDTHS[name]
        res.append((name, cin, cout, h, w, 1 if name[-1] == "b" else 3, name[-1] == "a", False))
    return res


def vgg_layers():
    res, h, w = [], H0, W0
    for idx, cin, cout, pool in CN.VGG16_CONVS:
        res.append((f"features.{idx}", cin, cout, h, w, 3, idx != 28, pool))
        h, w = CN.out_size(h, w, pool)
    return res


def flops(layers, B):
    return sum(2.0 * k * k * cin * cout * h * w * B for _, cin, cout, h, w, k, _, _ in layers)


def torch_superpoint(enc, image):
    x = image
    for name, pool in CN.SUPERPOINT_ENCODER:
        x = torch_layer(x, *enc.params[name], True, pool)
    return (torch_layer(torch_layer(x, *enc.params["convPa"], True, False), *enc.params["convPb"], False, False),
            torch_layer(torch_layer(x, *enc.params["convDa"], True, False), *enc.params["convDb"], False, False))


def torch_vgg(trunk, x):
    for idx, _, _, pool in CN.VGG16_CONVS:
        x = torch_layer(x, *trunk.params[idx], idx != 28, pool)
    return x


def he_state(table, g):
    sd = {}
    for name, cin, cout, k in table:
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[name + ".bias"] = torch.randn(cout, generator=g) * 0.1
    return sd


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_convnet.py measures on the GPU: no HIP device is available")
    torch.backends.cudnn.allow_tf32 = False
    g = torch.Generator().manual_seed(7)
    sp, vg = superpoint_layers(), vgg_layers()
    enc = CN.SuperPointEncoder(he_state([(n, ci, co, 1 if n in ("convPb", "convDb") else 3) for n, (ci, co) in CN.SUPERPOINT_WIDTHS.items()], g))
    trunk = CN.VGG16Trunk(he_state([(f"backbone.{i}", ci, co, 3) for i, ci, co, _ in CN.VGG16_CONVS], g))
    shapes = {}
    for name, *shape in sp + vg:
        shapes.setdefault(tuple(shape), []).append(name)
    rows = []
    for B in (1, 8):
        for (cin, cout, h, w, k, relu, pool), names in shapes.items():
            x = torch.randn(B, cin, h, w, generator=g).cuda()
            wt = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).cuda()
            bs = (torch.randn(cout, generator=g) * 0.1).cuda()
            out = torch.empty(B * cout * h * w, dtype=torch.float32, device="cuda")
            diff = float((CN.conv2d(x, wt, bs, relu, pool, out=out) - torch_layer(x, wt, bs, relu, pool)).abs().max())
            row = {"what": "layer", "layers": names, "B": B, "Cin": cin, "Cout": cout, "H": h, "W": w, "k": k, "pool": pool}
            row.update(alternate({"hip": lambda: CN.conv2d(x, wt, bs, relu, pool, out=out), "torch_conv2d": lambda: torch_layer(x, wt, bs, relu, pool)}))
            floor = 2.0 * k * k * cin * cout * h * w * B / PEAK * 1e3
            row.update({"mfma_floor_ms": round(floor, 4), "fraction_of_floor": round(floor / row["hip"]["median_ms"], 3),
                        "hip_over_torch": round(row["hip"]["median_ms"] / row["torch_conv2d"]["median_ms"], 3),
                        "max_abs_difference": float(f"{diff:.3g}")})
            rows.append(row)
            del x, wt, bs, out
        image = torch.rand(B, 1, H0, W0, generator=g).cuda()
        rgb = torch.randn(B, 3, H0, W0, generator=g).cuda()
        for what, layers, fns, diff in (
                ("superpoint_encoder", sp, {"hip": lambda: enc(image), "torch_conv2d": lambda: torch_superpoint(enc, image)},
                 lambda: float((enc(image)[1] - torch_superpoint(enc, image)[1]).abs().max())),
                ("vgg16_trunk", vg, {"hip": lambda: trunk(rgb), "torch_conv2d": lambda: torch_vgg(trunk, rgb)},
                 lambda: float((trunk(rgb) - torch_vgg(trunk, rgb)).abs().max()))):
            d = diff()
            row = {"what": what, "B": B, "H": H0, "W": W0, "gflop": round(flops(layers, B) / 1e9, 2)}
            row.update(alternate(fns))
            floor = flops(layers, B) / PEAK * 1e3
            row.update({"mfma_floor_ms": round(floor, 4), "fraction_of_floor": round(floor / row["hip"]["median_ms"], 3),
                        "hip_over_torch": round(row["hip"]["median_ms"] / row["torch_conv2d"]["median_ms"], 3),
                        "max_abs_difference": float(f"{d:.3g}")})
            rows.append(row)
    print(json.dumps({
        "what": "splatloc_amd.convnet (HIP implicit GEMM on the exact-f32 MFMA, one launch per layer, no host wait) vs "
                "torch.nn.functional.conv2d (+ relu, + max_pool2d) in float32 on the same device, on MI355X; "
                f"{REPS} alternating rounds in one process after a warm-up; ms per call, device events around {INNER} calls per sample; "
                f"mfma_floor_ms = 2 k k Cin Cout H W B over {PEAK / 1e12:.1f} TF",
        "status": "measured",
        "tiles": CN.tiles(),
        "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
