"""Code generation of csrc/fusion.hip, from the compiler's own report and the gfx950 assembly (cross-compiled; no GPU): no scratch
and no spills in any kernel, the feature rows move as 16-byte accesses per lane, and the translation unit is compiled without FP
contraction (the reference's operations round one by one)."""
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
    asm = str(tmp_path_factory.mktemp("fusion") / "fusion.s")
    flags = [f for f in B._flags("fusion.hip") if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, "fusion.hip"), "-o", asm], capture_output=True, text=True)
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
    return usage, bodies


def test_fusion_is_built_without_contraction():
    assert "fusion.hip" in B.SOURCES and "fusion.hip" in B.NO_CONTRACT
    assert "-ffp-contract=off" in B._flags("fusion.hip")


def test_no_scratch_and_no_spills_in_any_fusion_kernel(compiled):
    usage, _ = compiled
    kernels = {k: v for k, v in usage.items() if "fusion_" in k}
    # integrate; min/max, level, set level, count, extract, gather
    assert len(kernels) == 7, sorted(kernels)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    integrate = next(v for k, v in kernels.items() if "fusion_integrate_kernel" in k)
    assert integrate["Occupancy"] == 8 and integrate["VGPRs"] <= 64, integrate


def test_feature_rows_move_as_16_byte_accesses(compiled):
    _, bodies = compiled
    integrate = next(b for k, b in bodies.items() if "fusion_integrate_kernel" in k)
    gather = next(b for k, b in bodies.items() if "fusion_gather_kernel" in k)
    # the volume row and the image row are loaded and the volume row is stored with 16-byte instructions
    assert len(re.findall(r"\bglobal_load_dwordx4\b", integrate)) >= 2, re.findall(r"global_load_\w+", integrate)
    assert len(re.findall(r"\bglobal_store_dwordx4\b", integrate)) >= 1, re.findall(r"global_store_\w+", integrate)
    assert "global_load_dwordx4" in gather and "global_store_dwordx4" in gather

