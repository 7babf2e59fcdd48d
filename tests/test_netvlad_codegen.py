"""The compiler's own resource report for csrc/netvlad_head.hip (`-Rpass-analysis=kernel-resource-usage`, read the way
tests/test_codegen_budget.py reads it; hipcc cross-compiles gfx950 without a GPU): nothing in scratch, no VGPR or SGPR spill in any
kernel of the file, and no kernel with more LDS than its arrays declare.  The aggregation kernel prefetches a step of 24 rows per
thread and the projection kernel a chunk of 20 floats: a spill there would put the prefetch into scratch memory.  Every kernel is
held at the waves per SIMD it had before the file took its accumulator layout, step of four k and projection staging from
csrc/mfma_tile.h (HISTORY.md §35)."""
from tests.test_codegen_budget import _usage

# kernel -> bytes of LDS its __shared__ arrays declare
#   assign          score_w tile 64 x 36, xh tile 32 x 64, scores 64 x 65, norm partials 4 x 64, inv 64, sums 64 floats
#   aggregate       (32 xh + 64 a rows) x 68 floats
#   finish          64 sums of a, 16 x 64 column partials, 64 totals
#   project         (32 x + 128 weight rows) x 36 floats
#   project_finish  four wave partials
DECLARED = {
    "netvlad_assign_kernel": (64 * 36 + 32 * 64 + 64 * 65 + 4 * 64 + 64 + 64) * 4,
    "netvlad_aggregate_kernel": (32 + 64) * 68 * 4,
    "netvlad_finish_kernel": (64 + 16 * 64 + 64) * 4,
    "netvlad_project_kernelILb0E": (32 + 128) * 36 * 4,
    "netvlad_project_kernelILb1E": (32 + 128) * 36 * 4,
    "netvlad_project_finish_kernel": 4 * 4,
}


# kernel -> waves per SIMD
WAVES = {
    "netvlad_assign_kernel": 4,
    "netvlad_aggregate_kernel": 6,
    "netvlad_finish_kernel": 8,
    "netvlad_project_kernelILb0E": 3,
    "netvlad_project_kernelILb1E": 6,
    "netvlad_project_finish_kernel": 8,
}


def _find(usage, key):
    hits = [v for k, v in usage.items() if key in k]
    assert len(hits) == 1, (key, list(usage))
    return hits[0]


def test_no_scratch_and_no_spills_in_any_kernel():
    u = _usage("netvlad_head.hip")
    assert len(u) == len(DECLARED), list(u)
    for name, k in u.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


def test_lds_is_no_more_than_declared():
    u = _usage("netvlad_head.hip")
    for key, lds in DECLARED.items():
        k = _find(u, key)
        assert k["LDS Size"] <= lds, (key, k, lds)
    # two projection workgroups per CU fit by LDS and by registers
    for key in ("netvlad_project_kernelILb0E", "netvlad_project_kernelILb1E"):
        k = _find(u, key)
        assert 2 * k["LDS Size"] <= 160 * 1024 and k["Occupancy"] >= 2, (key, k)


def test_every_kernel_keeps_its_waves_per_simd():
    u = _usage("netvlad_head.hip")
    assert sorted(WAVES) == sorted(DECLARED)
    for key, waves in WAVES.items():
        k = _find(u, key)
        assert k["Occupancy"] >= waves, (key, k, waves)
