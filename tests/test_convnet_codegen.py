"""The compiler's own resource report for csrc/conv2d.hip (`-Rpass-analysis=kernel-resource-usage`, read the way
tests/test_codegen_budget.py reads it; hipcc cross-compiles gfx950 without a GPU): nothing in scratch, no VGPR or SGPR spill in any
kernel of the file, and no kernel with more LDS than its arrays declare.  The convolution kernel holds 64 accumulator registers and
prefetches a chunk of 16 patch and up to 20 weight values per thread: a spill there would put the prefetch into scratch memory.  The
3x3 kernels are held at 2 waves per SIMD and the 1x1 kernels at 3, what each had with its own copy of the accumulator layout that is
now csrc/mfma_tile.h's (HISTORY.md §35)."""
from tests.test_codegen_budget import _usage

# kernel -> bytes of LDS its __shared__ arrays declare: the patch, 8 planes of 10 x 34 pixels at a plane stride of 352 floats, and
# the weight slab, 64 rows at a stride of 74 floats (both kernel sizes stage the same arrays)
CONV_LDS = (8 * 352 + 64 * 74) * 4
DECLARED = {
    "conv2d_kernelILi3ELb0E": CONV_LDS,
    "conv2d_kernelILi3ELb1E": CONV_LDS,
    "conv2d_kernelILi1ELb0E": CONV_LDS,
    "conv2d_kernelILi1ELb1E": CONV_LDS,
    "netvlad_preprocess_kernel": 0,
}


def _find(usage, key):
    hits = [v for k, v in usage.items() if key in k]
    assert len(hits) == 1, (key, list(usage))
    return hits[0]


def test_no_scratch_and_no_spills_in_any_kernel():
    u = _usage("conv2d.hip")
    assert len(u) == len(DECLARED), list(u)
    for name, k in u.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


def test_lds_is_no_more_than_declared():
    u = _usage("conv2d.hip")
    for key, lds in DECLARED.items():
        k = _find(u, key)
        assert k["LDS Size"] <= lds, (key, k, lds)
    # two convolution workgroups per CU fit by LDS and by registers; the 1x1 kernels, with a ninth of the weight prefetch, fit three
    for key in DECLARED:
        if key.startswith("conv2d"):
            k = _find(u, key)
            assert 2 * k["LDS Size"] <= 160 * 1024 and k["Occupancy"] >= (3 if "ILi1E" in key else 2), (key, k)
