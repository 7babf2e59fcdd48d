"""tinycudann.Encoding timing on the office_0 hash grid (16 levels x 2 features, 2^19 entries, desired resolution 108: a 22 MB
table).  HIP events around the encoding calls alone (no allocation inside the timed region beyond torch's cached blocks):
python tools/grid_encoding_time.py > profiles/grid_encoding_time.json"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import tinycudann as tcnn  # noqa: E402

CFG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "per_level_scale": float(np.exp2(np.log2(108 / 16) / 15))}
REPS = 50


def _time(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


enc = tcnn.Encoding(3, CFG, dtype=torch.float)
with torch.no_grad():
    enc.params.uniform_(-1, 1)
lay = enc.layout
rows = []
for N in (256, 1_000_000):
    x = torch.rand((N, 3), generator=torch.Generator().manual_seed(N)).cuda()
    g = torch.randn((N, lay.n_output_dims), device="cuda")
    xg = x.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            enc(x)

    def fwd_bwd_params():
        enc.params.grad = None
        enc(x).backward(g)

    def fwd_bwd_both():
        enc.params.grad = None
        enc(xg).backward(g)

    row = {"N": N, "forward_ms": round(_time(fwd), 4), "forward_backward_params_ms": round(_time(fwd_bwd_params), 4),
           "forward_backward_params_and_input_ms": round(_time(fwd_bwd_both), 4),
           "gathered_bytes_per_point": lay.n_levels * 8 * lay.n_features_per_level * 4}
    row["forward_gather_GBps"] = round(N * row["gathered_bytes_per_point"] / (row["forward_ms"] * 1e-3) / 1e9, 1)
    rows.append(row)
print(json.dumps({"what": "tinycudann.Encoding (HIP) on MI355X, office_0 hash grid, ms per call: HIP events over "
                  f"{REPS} calls after 1 warm-up; backward times include the torch.zeros of dL/dparams",
                  "table_MB": round(lay.n_params * 4 / 1e6, 2), "rows": rows}, indent=1))
