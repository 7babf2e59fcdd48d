"""Code generation of csrc/decoder.hip, from the compiler's own report and the gfx950 assembly (cross-compiled; no GPU): no scratch
and no spills anywhere, the LDS and occupancy DESIGN.md §18 declares for the 32-128-128-128-256 decoder, exact-f32 MFMA in the
forward and the backward, and no compare-and-swap loop."""
import os
import re
import shutil
import subprocess

import pytest

from splatloc_amd import build as B


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = str(tmp_path_factory.mktemp("decoder") / "decoder.s")
    flags = [f for f in B._flags("decoder.hip") if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, "decoder.hip"), "-o", asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    bodies = {}
    text = open(asm).read()
    for name in usage:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*s_endpgm" % re.escape(name), text, re.S | re.M)
        assert m, name
        bodies[name] = m.group(1)
    return usage, bodies, text


def test_no_scratch_and_no_spills_in_any_decoder_kernel(compiled):
    usage, _, _ = compiled
    kernels = {k: v for k, v in usage.items() if "decoder_" in k}
    # forward: D {2, 3} x F {1, 2, 4, 8} x tile height {32, 64}; backward, reduce, Adam
    assert len(kernels) == 16 + 3, sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)


def test_lds_and_occupancy_of_the_reference_configuration(compiled):
    """two workgroups of four waves per CU (2 waves per SIMD) for every MFMA kernel, i.e. at most 80 KiB of LDS per
    workgroup and at most 256 registers (VGPRs + AGPRs) per lane."""
    usage, _, _ = compiled
    fwd64 = next(v for k, v in usage.items() if "decoder_fwd_kernelILi3ELi2ELi2E" in k)
    fwd32 = next(v for k, v in usage.items() if "decoder_fwd_kernelILi3ELi2ELi1E" in k)
    bwd = next(v for k, v in usage.items() if "decoder_bwd_kernel" in k)
    assert fwd64["LDS Size"] == 2 * 64 * 132 * 4 + 64 * 8 * 4 + 64 * 4 * 4 == 70_656
    assert fwd32["LDS Size"] == 35_328
    assert bwd["LDS Size"] == 32 * 260 * 4 + 2 * 32 * 132 * 4 + 32 * 4 == 67_200
    for k in (fwd64, fwd32, bwd):
        assert 2 * k["LDS Size"] <= 160 * 1024
        assert k["VGPRs"] + k["AGPRs"] <= 256 and k["Occupancy"] >= 2, k


def test_every_instantiation_keeps_its_waves_per_simd(compiled):
    """What each kernel had with its own copy of the accumulator layout and of the step of four k that are now csrc/mfma_tile.h's
    (HISTORY.md §35): every forward of tile height 64 at 2 waves per SIMD, every forward of tile height 32 at 4, the backward at 2
    and within 115 VGPRs, and none above 256 registers per lane."""
    usage, _, _ = compiled
    fwd = {k: v for k, v in usage.items() if "decoder_fwd_kernel" in k}
    tall = [v for k, v in fwd.items() if re.search(r"decoder_fwd_kernelILi\dELi\dELi2EE", k)]
    low = [v for k, v in fwd.items() if re.search(r"decoder_fwd_kernelILi\dELi\dELi1EE", k)]
    assert len(tall) == 8 and len(low) == 8, sorted(fwd)
    for v in tall:
        assert v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, v
    for v in low:
        assert v["Occupancy"] >= 4 and v["VGPRs"] + v["AGPRs"] <= 256, v
    bwd = next(v for k, v in usage.items() if "decoder_bwd_kernel" in k)
    assert bwd["Occupancy"] >= 2 and bwd["VGPRs"] <= 115 and bwd["VGPRs"] + bwd["AGPRs"] <= 256, bwd


def test_mfma_in_forward_and_backward_and_no_compare_and_swap(compiled):
    _, bodies, text = compiled
    for name, body in bodies.items():
        if "decoder_fwd_kernel" in name or "decoder_bwd_kernel" in name:
            assert "v_mfma_f32_32x32x2_f32" in body, name
    assert "cmpswap" not in text
