"""Code generation of csrc/fusion_mesh.hip, from the compiler's own report and the gfx950 assembly (cross-compiled; no GPU), as
tests/test_fusion_codegen.py does for fusion.hip: three kernels, no scratch and no spills (a cell's table row is picked apart with
constant shifts, never indexed dynamically), full occupancy, the faces pass fetches a row with one global_load_dwordx4, and the translation unit is compiled without
FP contraction (the normals round operation by operation)."""
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
    asm = str(tmp_path_factory.mktemp("fusion_mesh") / "fusion_mesh.s")
    flags = [f for f in B._flags("fusion_mesh.hip") if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, "fusion_mesh.hip"), "-o", asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    bodies = {}
    text = open(asm).read()
    for name in usage:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*s_endpgm" % re.escape(name), text, re.S | re.M)
        assert m, name
        bodies[name] = m.group(1)
    return usage, bodies


def test_mesh_is_built_without_contraction():
    assert "fusion_mesh.hip" in B.SOURCES and "fusion_mesh.hip" in B.NO_CONTRACT
    assert "-ffp-contract=off" in B._flags("fusion_mesh.hip")


def test_three_kernels_without_scratch_at_full_occupancy(compiled):
    usage, _ = compiled
    kernels = {k: v for k, v in usage.items() if "fusion_mesh_" in k}
    assert len(kernels) == 3 and len(usage) == 3, sorted(usage)      # count, faces, normals
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["Occupancy"] == 8 and v["VGPRs"] <= 64, (k, v)


def test_table_row_is_one_load_and_normals_divide_exactly(compiled):
    _, bodies = compiled
    faces = next(b for k, b in bodies.items() if "fusion_mesh_faces_kernel" in k)
    normals = next(b for k, b in bodies.items() if "fusion_mesh_normals_kernel" in k)
    # a vector load of the row (s_load_dwordx4 would be the kernel's arguments, not the table)
    assert len(re.findall(r"\bglobal_load_dwordx4\b", faces)) == 1, sorted(set(re.findall(r"\w+_load_\w+", faces)))
    assert not re.search(r"\bglobal_load_(ubyte|sbyte|ushort|dwordx3)\b", faces), sorted(set(re.findall(r"\w+_load_\w+", faces)))
    # three vertices at most per voxel, IEEE divisions (rounding itself is pinned by the bit-equality tests on the device)
    assert len(re.findall(r"\bv_div_fixup_f32", normals)) == 12          # per vertex: the quotient q and three components
