"""Times the NetVLAD head (splatloc_amd/netvlad.py, csrc/netvlad_head.hip) against the same head written with torch operators on
the device, at the layer's own shape D = 512, K = 64, N = 1200 (a 30 x 40 map) with an O = 4096 whitening, for B = 1 and B = 8:
each stage separately (assign, aggregate with both normalisations, project) and the whole head.  The torch side is timed in two
forms: hloc's literal layer ((a.unsqueeze(1) * (x.unsqueeze(2) - c)).sum(-1), which materialises a [B, D, K, N] tensor) and the
GEMM form of the contract (two matmuls), so that the comparison does not rest on the literal form's memory traffic.

For `project` the JSON also holds the byte floor 4 * O * I bytes over the MI355X's measured float4 copy rate (6.29 TB/s), the
fraction of that floor the kernel achieves (floor / time), and B = 8 against B = 1: the weights are read once per call.

The implementations alternate in one process, REPS rounds after a warm-up of every shape; device events around INNER calls per
sample; medians and the spread per row.  Before anything is timed the outputs are compared.

    python tools/time_netvlad_head.py > profiles/netvlad_head_time.json
"""
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from splatloc_amd import netvlad as NV  # noqa: E402

REPS = 10
INNER = 5
D, K, N, O = 512, 64, 1200, 4096
COPY_RATE = 6.29e12   # bytes / s, measured float4 copy


def torch_assign(x, w, b):
    xh = F.normalize(x, p=2, dim=1)
    return F.softmax(F.conv1d(xh, w[:, :, None], b), dim=1), xh


def torch_aggregate_literal(a, xh, c):
    desc = (a.unsqueeze(1) * (xh.unsqueeze(2) - c.unsqueeze(0).unsqueeze(-1))).sum(-1)
    return F.normalize(F.normalize(desc, p=2, dim=1).reshape(a.shape[0], -1), p=2, dim=1)


def torch_aggregate_gemm(a, xh, c):
    desc = torch.bmm(xh, a.transpose(1, 2)) - c.unsqueeze(0) * a.sum(2).unsqueeze(1)
    return F.normalize(F.normalize(desc, p=2, dim=1).reshape(a.shape[0], -1), p=2, dim=1)


def torch_project(v, W, wb):
    return F.normalize(F.linear(v, W, wb), p=2, dim=1)


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_netvlad_head.py measures on the GPU: no HIP device is available")
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(K, D, generator=g) * 2.0).cuda()
    sb = (torch.randn(K, generator=g) * 0.5).cuda()
    c = (torch.randn(D, K, generator=g) / D ** 0.5).cuda()
    W = (torch.randn(O, D * K, generator=g) / (D * K) ** 0.5).cuda()
    wb = (torch.randn(O, generator=g) * 0.1).cuda()
    head = NV.NetVLADHead(w, c, sb, W, wb)
    rows, project_ms = [], {}
    for B in (1, 8):
        x = (torch.randn(B, D, N, generator=g) * (0.5 + torch.rand(B, 1, N, generator=g))).cuda()
        a, inv = head.assign(x)
        v = head.vlad(x)
        ta, txh = torch_assign(x, w, sb)
        tv = torch_aggregate_gemm(ta, txh, c)
        agree = {"assign": float((a - ta).abs().max()), "v": float((v - tv).abs().max()),
                 "v_literal": float((v - torch_aggregate_literal(ta, txh, c)).abs().max()),
                 "y": float((head(x) - torch_project(tv, W, wb)).abs().max())}
        ws = head._workspace(B, N)
        sides = {
            "assign": {"hip": lambda: head.assign(x), "torch_operators": lambda: torch_assign(x, w, sb)},
            "aggregate": {"hip": lambda: head._aggregate(x, a, inv, NV.INTRANORM | NV.L2NORM, ws),
                          "torch_operators_literal": lambda: torch_aggregate_literal(ta, txh, c),
                          "torch_operators_gemm": lambda: torch_aggregate_gemm(ta, txh, c)},
            "project": {"hip": lambda: head.project(v), "torch_operators": lambda: torch_project(tv, W, wb)},
            "head": {"hip": lambda: head(x),
                     "torch_operators_literal": lambda: torch_project(torch_aggregate_literal(*torch_assign(x, w, sb), c), W, wb),
                     "torch_operators_gemm": lambda: torch_project(torch_aggregate_gemm(*torch_assign(x, w, sb), c), W, wb)},
        }
        for what, fns in sides.items():
            for fn in fns.values():      # warm-up of every shape
                fn()
                fn()
            ms = {k: [] for k in fns}
            for _ in range(REPS):
                for k, fn in fns.items():
                    ms[k].append(timed(fn, INNER))
            row = {"what": what, "B": B, "D": D, "K": K, "N": N, "O": O}
            row.update({k: stats(v_) for k, v_ in ms.items()})
            if what == "project":
                floor_ms = 4.0 * O * D * K / COPY_RATE * 1e3
                med = row["hip"]["median_ms"]
                project_ms[B] = med
                row.update({"weight_bytes": 4 * O * D * K, "byte_floor_ms": round(floor_ms, 4),
                            "fraction_of_byte_floor": round(floor_ms / med, 3),
                            "torch_fraction_of_byte_floor": round(floor_ms / row["torch_operators"]["median_ms"], 3)})
            rows.append(row)
        rows.append({"what": "max abs difference, HIP against the torch operators", "B": B, **{k: float(f"{e:.3g}") for k, e in agree.items()}})
    print(json.dumps({
        "what": "NetVLADHead (HIP, one launch sequence per batch, no host wait) vs the same head with torch operators on the device, on "
                f"MI355X; {REPS} alternating rounds in one process after a warm-up; ms per call, device events around {INNER} calls per "
                f"sample; byte_floor_ms = 4 O I bytes over the measured copy rate {COPY_RATE / 1e12:.2f} TB/s",
        "status": "measured",
        "project_B8_over_B1": round(project_ms[8] / project_ms[1], 3),
        "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
