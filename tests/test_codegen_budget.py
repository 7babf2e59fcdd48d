"""Register / scratch / occupancy budget of the two compositing kernels, read from the compiler's own report
(`-Rpass-analysis=kernel-resource-usage`; hipcc cross-compiles gfx950 without a GPU).  Round 4 traced two regressions of
the headline kernel to code generation nobody had looked at — a "prefetch" whose registers were spilled right behind the
loads, an epilogue with a wait between every two stores — so the numbers the design depends on (HISTORY.md §9) are
pinned here: a source or toolchain change that costs a wave per SIMD or re-introduces scratch traffic fails on the CPU."""
import functools
import os
import re
import shutil
import subprocess

import pytest

from splatloc_amd import build as B


@functools.lru_cache(maxsize=None)     # one compilation per file, whichever tests read its report
def _usage(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = [f for f in B._flags(src) if f not in ("-fPIC",)]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def _kernel(usage, prefix):
    hits = {k: v for k, v in usage.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, list(usage))
    return next(iter(hits.values()))


def test_forward_kernels_have_no_scratch_and_keep_their_occupancy():
    u = _usage("composite_fwd.hip")
    fwd = {int(re.search(r"composite_fwd_kernelILi(\d+)E", k).group(1)): v for k, v in u.items() if "composite_fwd_kernel" in k}
    narrow = {int(re.search(r"composite_fwd_narrow_kernelILi(\d+)E", k).group(1)): v for k, v in u.items() if "composite_fwd_narrow_kernel" in k}
    mixed = {int(re.search(r"composite_fwd_mixed_kernelILi(\d+)E", k).group(1)): v for k, v in u.items() if "composite_fwd_mixed_kernel" in k}
    assert sorted(fwd) == [8, 16, 32, 35] and sorted(narrow) == [1, 2, 3, 4] and sorted(mixed) == [1, 2, 3, 4]
    for nc, k in list(fwd.items()) + list(narrow.items()) + list(mixed.items()):
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (nc, k)
    for nc in (1, 2, 3, 4):
        # the declared budget, __launch_bounds__(WAVE, 7): <= 72 registers, >= 7 waves per SIMD (today's toolchain: 64 / 8)
        assert narrow[nc]["VGPRs"] <= 72 and narrow[nc]["Occupancy"] >= 7, (nc, narrow[nc])
        # one workgroup of four waves per tile / per quadrant of a long list: five workgroups per CU by LDS, never fewer by registers
        assert mixed[nc]["VGPRs"] <= 96 and mixed[nc]["Occupancy"] >= 5 and mixed[nc]["LDS Size"] <= 28 * 1024, (nc, mixed[nc])
    assert fwd[35]["VGPRs"] <= 96 and fwd[35]["Occupancy"] >= 5, fwd[35]      # the headline layout: 5 waves per SIMD
    assert fwd[35]["LDS Size"] <= 5700, fwd[35]                               # 28 workgroups per CU by LDS


def test_wide_forward_kernels_of_the_other_layouts_keep_their_occupancy():
    """composite_fwd_kernel<8>, <16>, <32>: the chunked passes of a generic channel count and the three fixed layouts beside the
    headline one.  They share every step of the walk with the narrow kernels (HISTORY.md §21): nothing in scratch, and no fewer
    waves per SIMD than each had with its own copy of those steps (74 / 102 / 91 VGPRs: 6 / 4 / 5 waves)."""
    u = _usage("composite_fwd.hip")
    for nc, waves in ((8, 6), (16, 4), (32, 5)):
        k = _kernel(u, f"_ZN2sr20composite_fwd_kernelILi{nc}EE")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (nc, k)
        assert k["Occupancy"] >= waves, (nc, k)


def test_backward_kernels_stay_within_their_register_budget():
    u = _usage("composite_bwd.hip")
    wide = _kernel(u, "_ZN2sr20composite_bwd_kernelILi35ELb0ELb0ELb1E")        # <35, normal mode, butterfly variant, with depth / alpha>
    assert wide["VGPRs"] <= 128 and wide["Occupancy"] == 4, wide
    assert wide["VGPRs Spill"] <= 3 and wide["ScratchSize"] <= 12, wide        # (the spilled values live outside the loops: HISTORY.md §9)
    for nc in (1, 2, 3):                                                        # the butterfly variants of the narrow layouts: full occupancy, no scratch
        k = _kernel(u, f"_ZN2sr20composite_bwd_kernelILi{nc}ELb0ELb0ELb1E")
        assert k["Occupancy"] == 8 and k["ScratchSize"] == 0, (nc, k)
    ref = _kernel(u, "_ZN2sr20composite_bwd_kernelILi4ELb0ELb1ELb1E")          # SplatLoc's own layout, small-panel variant
    assert ref["ScratchSize"] == 0 and ref["Occupancy"] >= 5, ref
    refine = _kernel(u, "_ZN2sr20composite_bwd_kernelILi3ELb0ELb0ELb0E")       # color_refinement: 3 channels, no depth / alpha terms
    assert refine["ScratchSize"] == 0 and refine["Occupancy"] == 8, refine
    # every other instantiation <NC, DET, SP> (AUX = true), each at the waves per SIMD and the scratch it had before the kernel took its
    # frame, alpha test, partition and segment records from composite_common.h (HISTORY.md §22)
    others = {(8, 0, 0): (7, 0), (8, 0, 1): (5, 0), (16, 0, 0): (5, 0), (4, 1, 1): (5, 0), (4, 1, 0): (7, 0), (8, 1, 0): (6, 0),
              (8, 1, 1): (4, 0), (16, 1, 0): (4, 0), (32, 0, 0): (4, 8),
              (1, 1, 0): (8, 0), (2, 1, 0): (8, 0), (3, 1, 0): (8, 0), (4, 0, 0): (8, 0), (32, 1, 0): (4, 12), (35, 1, 0): (4, 20)}
    for (nc, det, sp), (waves, scratch) in others.items():
        k = _kernel(u, f"_ZN2sr20composite_bwd_kernelILi{nc}ELb{det}ELb{sp}ELb1E")
        assert k["Occupancy"] >= waves and k["ScratchSize"] <= scratch, ((nc, det, sp), k)
    assert len([k for k in u if "composite_bwd_kernel" in k]) == 6 + len(others), list(u)   # all 21 are named above


def test_per_gaussian_backward_kernels_keep_their_occupancy():
    """The three kernels built from projection_bwd.h (HISTORY.md §19): nothing in scratch, the camera reduction's LDS allocated
    once per kernel (s_pose[4][32] + s_last), and no instantiation below the waves per SIMD it had with its own copy of the
    derivative.  window_joint_bwd_kernel<4> sits two registers under its boundary (166 of 168): the occupancy assertion is
    what holds it there."""
    pre, cam, joint = _usage("preprocess_bwd.hip"), _usage("camera_bwd.hip"), _usage("window_joint_bwd.hip")
    for u in (pre, cam, joint):
        for name, k in u.items():
            assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (name, k)
    # preprocess_bwd_kernel<POSE, RAW, TQ>
    occ = {(0, 1, 0): 3, (1, 0, 4): 2, (1, 0, 1): 2, (1, 0, 0): 3, (0, 0, 4): 2, (0, 0, 1): 3, (0, 0, 0): 3}
    for (pose, raw, tq), waves in occ.items():
        k = _kernel(pre, f"_ZN2sr21preprocess_bwd_kernelILb{pose}ELb{raw}ELi{tq}EE")
        assert k["Occupancy"] >= waves and k["LDS Size"] == (516 if pose else 0), ((pose, raw, tq), k)
    for tq in (4, 1, 0):
        k = _kernel(joint, f"_ZN2sr23window_joint_bwd_kernelILi{tq}EE")
        assert k["Occupancy"] >= 3 and k["LDS Size"] == 516, (tq, k)
    k = _kernel(cam, "_ZN2sr17camera_bwd_kernelE")
    assert k["Occupancy"] >= 8 and k["LDS Size"] == 516, k


def test_loss_stage_kernels_keep_their_occupancy_and_lds():
    """The loss stage's kernels since they share their block sums (reduce.h), one blur body and one L1 kernel: nothing in scratch,
    no spill, and no kernel below the waves per SIMD or above the LDS footprint it had with its own copy of each (refine_fwd_kernel
    then needed 115 VGPRs for 4 waves; LDS may only shrink)."""
    losses, densify, pose = _usage("losses.hip"), _usage("densify.hip"), _usage("pose.hip")
    pins = ((losses, "_ZN2sr17refine_fwd_kernelE", 4, 26192), (losses, "_ZN2sr17refine_bwd_kernelE", 6, 23792),
            (losses, "_ZN2sr19eval_metrics_kernelE", 6, 14576), (losses, "_ZN2sr19mapping_loss_kernelE", 8, 160),
            (losses, "_ZN2sr26mapping_loss_finish_kernelE", 8, 160), (losses, "_ZN2sr26eval_metrics_finish_kernelE", 8, 96),
            (densify, "_ZN2sr20isotropic_fwd_kernelE", 8, 64), (densify, "_ZN2sr23isotropic_finish_kernelE", 8, 0),
            (pose, "_ZN2sr26l1_rgbd_loss_window_kernelE", 8, 16))
    for u, name, waves, lds in pins:
        k = _kernel(u, name)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
        assert k["Occupancy"] >= waves and k["LDS Size"] <= lds, (name, k)
    assert _kernel(losses, "_ZN2sr17refine_fwd_kernelE")["VGPRs"] <= 115
    assert len(losses) == 6 and not [k for k in pose if "l1_rgbd_loss_kernel" in k], (list(losses), list(pose))


def test_model_update_kernels_keep_their_occupancy():
    """densify.hip since the scalar Adam element, the moments row, the group table and the Adam entry are each written once
    (HISTORY.md §32): the same nine kernels, and the seven of the model update with nothing in scratch, no spill, no LDS and the full
    8 waves per SIMD.  They are HBM-bound and hold no LDS, so occupancy and scratch are what their speed depends on.  VGPRs, each
    kernel with its own copy of those steps -> with the shared ones: adam_kernel 26 -> 26 (both forms), adam_quad_kernel
    46 -> 48 (both forms), densify_gather_kernel 38 -> 38, model_append_kernel 16 -> 16,
    densify_flags_kernel 25 -> 25.  The two isotropic kernels are pinned with the loss stage above."""
    u = _usage("densify.hip")
    assert len(u) == 9, list(u)
    for name in ("_ZN2sr11adam_kernelIJEEE", "_ZN2sr11adam_kernelIJPKjEEE", "_ZN2sr16adam_quad_kernelIJEEE",
                 "_ZN2sr16adam_quad_kernelIJPKjEEE", "_ZN2sr21densify_gather_kernelE", "_ZN2sr19model_append_kernelE",
                 "_ZN2sr20densify_flags_kernelE"):
        k = _kernel(u, name)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] == 0, (name, k)
        assert k["Occupancy"] >= 8, (name, k)
    assert len([k for k in u if "isotropic" in k]) == 2, list(u)


def test_scan_and_sort_kernels_keep_their_registers_and_lds():
    """The scan, radix-sort and tile-order kernels since they take their wave scan, workgroup scan and digit ranks from scan.h and
    one rank body (HISTORY.md §29): nothing in scratch, no spill, and no kernel above the VGPRs or the LDS footprint, or below the
    waves per SIMD, that it has with the shared forms.  While each carried its own copy the compiler reported (VGPRs / waves)
    44 / 8 and 36 / 8 for the one-pass scans, 92 / 5 and 124 / 4 for the sweeps and 16 / 8 for the tile order, the rest as below:
    the pins are the lower figures, so what the shared workgroup scan gained (a wave per SIMD in sort_sweep_kernel<8>) is held too."""
    sort, binning = _usage("scan_sort.hip"), _usage("binning.hip")
    pins = ((sort, "_ZN2sr19scan_onepass_kernelILb0EE", 42, 8, 32), (sort, "_ZN2sr19scan_onepass_kernelILb1EE", 34, 8, 32),
            (sort, "_ZN2sr20sort_hist_all_kernelILi8EE", 11, 8, 4096), (sort, "_ZN2sr20sort_hist_all_kernelILi16EE", 11, 8, 4096),
            (sort, "_ZN2sr17sort_sweep_kernelILi8EE", 74, 6, 4116), (sort, "_ZN2sr17sort_sweep_kernelILi16EE", 122, 4, 4116),
            (sort, "_ZN2sr19sort_scatter_kernelIjjEE", 108, 4, 37904), (sort, "_ZN2sr19sort_scatter_kernelIttEE", 108, 4, 29712),
            (sort, "_ZN2sr19sort_scatter_kernelItjEE", 108, 4, 29712), (binning, "_ZN2sr17tile_order_kernelE", 12, 8, 4160))
    for u, name, vgprs, waves, lds in pins:
        k = _kernel(u, name)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= vgprs and k["Occupancy"] >= waves and k["LDS Size"] <= lds, (name, k)


def test_retrieval_kernels_keep_their_occupancy_lds_and_scratch():
    """retrieval.hip since retrieval_kernel takes its accumulator layout, its step of four k and its staging from mfma_tile.h
    (HISTORY.md §35): no spill, and retrieval_kernel<VEC, RB> at no fewer waves per SIMD, no more LDS and no more scratch than it
    had with its own copy of each (159 / 219 / 86 / 138 VGPRs then; the two float4 forms kept 40 bytes per lane in scratch).  The
    merge and the two pose kernels: the full 8 waves, nothing in scratch."""
    u = _usage("retrieval.hip")
    assert len(u) == 7, list(u)
    for name, k in u.items():
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
    # <VEC, RB>: (waves per SIMD, LDS bytes, scratch bytes per lane)
    pins = {(1, 4): (2, 36864, 40), (0, 4): (1, 36864, 0), (1, 1): (4, 23040, 40), (0, 1): (3, 23040, 0)}
    for (vec, rb), (waves, lds, scratch) in pins.items():
        k = _kernel(u, f"_ZN2sr12_GLOBAL__N_116retrieval_kernelILb{vec}ELi{rb}EE")
        assert k["Occupancy"] >= waves and k["LDS Size"] <= lds and k["ScratchSize"] <= scratch, ((vec, rb), k)
    for name in ("retrieval_merge_kernel", "pose_errors_kernel", "pose_invert_kernel"):
        hits = [v for key, v in u.items() if name in key]
        assert len(hits) == 1, (name, list(u))
        assert hits[0]["Occupancy"] >= 8 and hits[0]["ScratchSize"] == 0, (name, hits[0])
