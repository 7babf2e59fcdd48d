#!/usr/bin/env python3
"""Regenerates profiles/README.md FROM the files under profiles/ — every number in it is read out of the file it is quoted
for (round 3's hand-written table drifted: the README said 4 492.6 us where the file said 4 192.16).  Descriptions without
numbers come from the table below; a file that is not listed there still gets a row ("(undescribed)").
usage: python tools/profiles_readme.py            (writes profiles/README.md)"""
import glob
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(ROOT, "profiles")

WHAT = [   # (file name regex, description; {placeholders} are filled by the extractors below)
    (r"r\d+_kernel_stats\.txt$", "`rocprofv3 --kernel-trace --stats` of the default bench (S2; round 3 on: window-batched, one launch sequence per 5 views): {kstats}"),
    (r"r\d+_ref_layout_kernel_stats\.txt$", "the same for `bench.py --workload S2-ref-layout` (500k, 640x480, C = 4): {kstats}"),
    (r"r\d+_pmc_hbm\.json$", "separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of the same command; HBM bytes per launch = 2 x FETCH (gfx950 correction) + WRITE: {hbm}"),
    (r"r\d+.*pmc_sq_counters.*\.json$", "SQ counter passes (`tools/pmc_passes.sh`) of the compositing kernels: {sq}"),
    (r"r\d+_timeline\.txt$", "kernel timeline of one step of the default bench (start, duration, idle gap): {timeline}"),
    (r"r\d+_ref_layout_timeline\.txt$", "kernel timeline of one window at the reference layout: {timeline}"),
    (r"r\d+_refine_step_timeline\.txt$", "kernel timeline of one `color_refinement` iteration under rocprofv3 (the live figures are in `r04_refine_idle*.json`): {timeline}"),
    (r"r\d+_bench_under_rocprof\.json$", "the bench line printed by the profiled run itself: {bench}"),
    (r"r\d+_bench.*\.json$", "bench line: {bench}"),
    (r"r\d+_stage_.*\.json$", "`bench.py --stage ...` line: {bench}"),
    (r"r\d+_clocks\.json$", "shader clock / socket power / throttle residency sampled at ~20 Hz by a separate process (amdsmi library) while bench.py ran >= 10 s of S2 windows (`tools/clock_trace.py`): {clocks}"),
    (r"r\d+_clocks_trace\.json$", "the thinned sample trace behind the clock summary"),
    (r"r\d+_grad_bars.*\.json$", "distribution of the absolute tolerance the full-size window gradients NEED (tensor-scale and per-row), normal and accurate mode, oracle modes 0 / 1 (`tools/grad_bar_probe.py`): {gradbars}"),
    (r"r\d+_refine_idle.*\.json$", "live GPU idle of a `color_refinement` iteration (`tools/refine_idle.py`): {idle}"),
    (r"r\d+_hostprof_.*\.txt$", "cProfile of the host side of a refinement / map step (`tools/hostprof_steps.py`)"),
    (r"r\d+_ab_probes\.txt$", "A/B and timing-probe log of the round (one box per block)"),
    (r"r\d+_knn\.json$", "`distCUDA2` wall times, brute force vs exact grid"),
    (r"^decoder_time\.json$", "fused FeatureDecoder against the composed path (`tinycudann.Encoding` + torch layers + `torch.optim.Adam`), HIP events, interleaved regions (`tools/decoder_time.py`): {decoder}"),
    (r"^fusion_time\.json$", "feature-TSDF fusion at office_0's size (21.9 M voxels x 256 channels, 640 x 480 frames) against the same update composed from torch operators, HIP events, interleaved regions (`tools/fusion_timing.py`): {fusion}"),
    (r"^fusion_mesh_time\.json$", "surface mesh at office_0's grid (21.9 M voxels) on a synthetic room TSDF, HIP events, interleaved regions beside a 1 GiB device copy (`tools/fusion_timing.py --mesh`): {fusionmesh}"),
    (r"^pnp_time\.json$", "absolute pose (`solve_pose`: P3P LO-RANSAC + Cauchy refinement) on planted scenes, HIP events (`tools/pnp_time.py`): {pnp}"),
    (r"^localize_time\.json$", "localisation (`tools/localize_time.py`), HIP events, interleaved medians: fused retrieval against `torch.einsum(...).topk` and the batched `Localizer.localize` against the per-query loop: {localize}"),
    (r"^image_ops_time\.json$", "frame preparation (`tools/time_image_ops.py`), HIP events, alternating medians, ms per call: `image_ops.compute_grad_masks` against the per-block loop of `Camera.compute_grad_mask` written with torch operators: {imageops}"),
    (r"^netvlad_head_time\.json$", "NetVLAD head (`tools/time_netvlad_head.py`), D = 512, K = 64, N = 1200, O = 4096, alternating medians of 10 rounds, ms per call, device events: `NetVLADHead` against the same head written with torch operators on the device (where two figures follow: hloc's literal form / the GEMM form); `project` with the byte floor 4 O I bytes over 6.29 TB/s: {nvhead}"),
    (r"^convnet_time\.json$", "convolution backbones (`tools/time_convnet.py`), 480 x 640 frames, alternating medians of 10 rounds, ms per call, device events: `convnet` against `torch.nn.functional.conv2d` (+ relu, + max_pool2d) in float32 on the device, with the MFMA floor 2 k k Cin Cout H W B over 157.3 TF: {convnet}"),
    (r"^superpoint_head_time\.json$", "SuperPoint head (`tools/time_superpoint_head.py`), 480 x 640 frames, alternating medians of 10 rounds, ms per call, device events (host clock to the end of a synchronise in brackets): `superpoint.detect` against the same head written with torch operators on the device, its `nonzero` wait included; `dense_descriptors` with the bytes it writes: {sphead}"),
    (r"^pose_window_time\.json$", "pose refinement of 8 query frames at 640x480, `pose.refine_poses` per `window` against the loop of 8 `pose.refine_pose` calls, ms per frame-iteration, host clock around a device synchronise, alternating regions (`tools/pose_window_time.py`): {posewindow}"),
    (r"^refine_bounded_time\.json$", "`training.refine_bounded` (no host wait for the instance count) against this tree's plain loop of `color_refinement_step` calls (not a build of the parent commit), us per iteration, host clock around a device synchronise, interleaved regions in one process (`tools/refine_bounded_time.py`): {refinebounded}"),
    (r"^joint_window_time\.json$", "one backward of a 5-view window that returns parameter AND camera gradients, ms per backward, host clock around a device synchronise, alternating regions (`tools/joint_window_time.py`): {jointwindow}"),
    (r"^matching_time\.json$", "2D-3D matching (`hungarian_solve` cost + exact assignment, batched solver, frustum candidates) against torch-CPU + scipy on the same host, HIP events (`tools/matching_time.py`): {matching}"),
    (r"^landmark_selection_time\.json$", "landmark selection (`gaussian_selectition`) at Replica scale on a synthetic room, HIP events per stage (`tools/landmark_selection_time.py`): {landmark}"),
    (r"r\d+_scene_lists.*\.json$", "one `color_refinement` iteration on a RECONSTRUCTED room (list-length distribution, per-kernel table; `tools/scene_lists.py`; suffix = the forced variant): {scenelists}"),
    (r"r\d+_scene.*\.json$", "`bench.py --stage scene`: the whole reconstruction schedule as one run (suffix: `replica_scale` = 180 key-frames of a 600k-Gaussian room, `radix_front_end` = SPLATRASTER_FRONT_END=0): {bench}{scene}"),
    (r"r\d+_ab_.*\.json$", "`tools/ab.py`: interleaved same-box A/B of variant libraries, paired statistics: {ab}"),
    (r"r\d+_bwd_profile\.txt$", "per-phase cycle counters of the wide backward's waves (`tools/bwd_prof.py`, `-DSR_BWD_PROFILE` variant from `tools/patches/r05_variants.patch`)"),
    (r"r\d+_lone_wave\.json$", "one wave alone on its SIMD walking one list of N entries (`tools/lone_wave.py`): us per 1 000 list entries of the narrow forward, one-wave vs four-wave team"),
    (r"r\d+_perview_idle.*\.json$", "the literal per-view drop-in loop (5 x `GaussianRasterizer.__call__` + backward) against the window: wall vs GPU busy time (`tools/perview_idle.py`): {perview}"),
    (r"r\d+_map_idle.*\.json$", "live GPU idle and raster / non-raster kernel split of one `training.map_step` (`tools/map_idle.py`): {mapidle}"),
    (r"r\d+_rccl_contact\.json$", "`tools/rccl_contact.py` on one MI355X: a world-size-1 `nccl` (RCCL) process group drives every collective call of the frame-parallel path (in-place span SUM, MAX, reduce-scatter + all-gather, header, broadcast_model): {rccl}"),
    (r"r\d+_bench_force_process_group.*\.json$", "`bench.py --gpus 1 --force-process-group`: the BASELINE step with its collectives issued on a world-size-1 RCCL group: {bench}"),
    (r"^bwd_setup_isa\.txt$", "set-up of one quadrant wave of the headline backward, parent against the pointer-walk form (DESIGN §13.8): instruction classes per basic block in front of the chunk loop (`tools/isa_blocks.py` on `hipcc -S`), the compiler's resource report"),
    (r"^bwd_setup_pmc\.json$", "`rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAVES` of the headline backward per launch, parent against the change, one run each: {setup_pmc}"),
    (r"^bwd_setup_kernel_stats\.txt$", "`rocprofv3 --kernel-trace --stats` of the default bench, parent (first listing) and change (second): {kstats2}"),
    (r"^bwd_setup_ab\.json$", "`tools/ab.py`, base = the change, variant `parent` = the parent commit's library (differences are parent minus change): {ab}; {setup_ab}"),
    (r"^front_end_kernel_stats\.txt$", "`rocprofv3 --kernel-trace --stats` of the default bench, parent (first listing) and the 16-bit tile-sort keys (second; DESIGN §3.1), us per launch: {fe_kstats}"),
    (r"^front_end_pmc_hbm\.json$", "separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of the same command for the radix front end's kernels, parent and change, and FETCH_SIZE of `payload_kernel` under the XCD-band mappings of `tools/patches/payload_xcd_band.patch`: {fe_pmc}"),
    (r"^front_end_ab\.json$", "`tools/ab.py`, base = the change (16-bit tile-sort keys), variants = the parent commit's library and the rejected XCD-band mappings of `payload_kernel` with and without the 16-bit keys (differences are variant minus change): {ab}; {fe_ab}"),
    (r"^payload_compact_kernel_stats\.txt$", "`rocprofv3 --kernel-trace --stats` of the default bench, parent (first listing) and the compact payload (second; DESIGN §3.1), us per launch: {pc_kstats}"),
    (r"^payload_compact_pmc_hbm\.json$", "separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs of the default bench, parent and change, for the payload and the two compositing kernels, and the live fraction of the window's tile instances read through `introspect.payload_state`: {pc_pmc}"),
    (r"^fwd_shared_steps_ab\.json$", "`tools/ab.py`, base = the change (the forward walkers' shared steps, HISTORY §21), variant `parent` = the parent commit's library (differences are parent minus change): {ab}; the other workloads, `--stage refine_step`, the `composite_fwd` stage in ms and cycles and the bit-for-bit comparison of the outputs under `other_runs` / `outputs_parent_vs_change`"),
    (r"^bwd_shared_contract_ab\.json$", "`tools/ab.py`, base = the change (the backward takes its frame, alpha test, partition and segment records from `composite_common.h`, HISTORY §22), variant `parent` = the parent commit's library (differences are parent minus change): {ab}; the other runs that were made, `--stage refine_step`, the `composite_bwd` stage in ms and cycles and the bit-for-bit comparison of outputs and deterministic-mode gradients under `other_runs` / `outputs_parent_vs_change`"),
    (r"^loss_shared_bodies_ab\.json$", "the loss stage's shared bodies (HISTORY §23) against the parent commit's library: interleaved pairs of fresh `bench.py --stage loss` / `refine_step` / `eval_rendering` / `pose_refine` processes on one box (200 steps, 20 warm-up), every run, and per stage the medians, the parent's spread and the paired difference (head minus parent) with its 95 % interval under `summary`; per-kernel means of one `rocprofv3 --kernel-trace --stats` run per side under `kernel_trace`"),
    (r"^scan_shared_ab\.json$", "the shared integer scans, ranks and selects of `csrc/scan.h` (HISTORY §29) against the parent commit's library: interleaved pairs of fresh `bench.py --stage raster` / `map_step` processes on one box (200 steps, 20 warm-up), every run, and per stage the medians, the parent's spread and the paired difference (head minus parent) with its 95 % interval under `summary`; per-kernel means of one `rocprofv3 --kernel-trace --stats` run per side and workload under `kernel_trace`; the rows of `tools/time_superpoint_head.py` and `tools/time_image_ops.py` with either library under `tools`; the counts of the bit-for-bit comparison under `bit_for_bit`"),
    (r"^activation_edges_ab\.json$", "the two activation fixes (HISTORY §31: `act_normalize_bwd` below the eps of normalize, the isotropic `d_scaling`) against the parent commit's library: eight interleaved pairs of fresh `bench.py --stage raster` / `map_step` processes in one session (200 steps, 20 warm-up), every run, and per stage the medians, the parent's own spread and the paired difference (head minus parent) with its 95 % interval under `summary`; the compiler's VGPR / scratch / occupancy figures of the nine touched kernels at parent and head; two earlier sessions (the header alone; a branching form that was not kept) under `earlier_sessions`"),
    (r"^workspace_carver_ab\.json$", "the host-side workspace carver (`Carver` in `csrc/common.h`, HISTORY §30; no kernel changes) against the parent commit's library: interleaved pairs of fresh `bench.py --stage raster` / `map_step` processes on one box (200 steps, 20 warm-up), every run, and per stage the medians, the parent's own spread and the paired difference (head minus parent) with its 95 % interval under `summary`"),
    (r"^dead_marks_share\.json$", "the forward's dead marks after one S2 window of five views, read through `introspect.payload_state` (`idead` against `imask`, bounded by `n_contrib_c`): {dm_share}"),
    (r"^dead_marks_share_room\.json$", "the same share on the reconstructed room of `tools/scene_lists.py`, its views rendered at C = 8 (colour table padded by zero columns) so that the wide forward marks: {dm_room}"),
    (r"^dead_marks_kernel_stats\.txt$", "`rocprofv3 --kernel-trace --stats` of the default bench, parent (first listing) and the dead marks as shipped (second; DESIGN §6.2b, §13.9), one run each, us per launch: {pc_kstats}"),
    (r"^dead_marks_ab\.json$", "`tools/ab.py`, base = the change (dead marks), variant `parent` = the parent commit's library (differences are parent minus change): {ab}"),
    (r"^payload_compact_ab.*\.json$", "`tools/ab.py`, base = the change (compact payload), variant `parent` = the parent commit's library (differences are parent minus change): {ab}; {pc_ab}"),
    (r"traffic\.json$", "per-stage HBM bytes per launch that `bench.py` replays as `roofline.traffic` (recorded workload / launch mode inside)"),
    (r"valu\.json$", "VALU / MFMA / SALU wave-instructions, busy fractions of the two compositing kernels per launch (replayed by `bench.py` as `frame_valu` / `roofline_valu`)"),
    (r"r01_v1_first_.*", "round 1: the first correct pipeline (per-value DPP reductions, no reach masks)"),
]


def _load(path):
    try:
        with open(path) as f:
            txt = f.read().strip()
        try:
            return json.loads(txt)
        except ValueError:
            return json.loads(next(ln for ln in txt.splitlines() if ln.startswith("{")))
    except Exception:  # noqa: BLE001
        return None


def kstats(path):
    rows = []
    for ln in open(path):
        m = re.match(r"(composite_(?:bwd|fwd)_kernel<[^>]*>)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)", ln)
        if m:
            rows.append(f"`{m.group(1)}` {float(m.group(4)):.2f} us avg over {m.group(2)} launches ({float(m.group(5)):.1f} %)")
    return "; ".join(rows[:3]) or "(no compositing kernel rows)"


def hbm(path):
    j = _load(path) or {}
    out = []
    for k, e in j.items():
        if "composite" in k and isinstance(e, dict) and "hbm_bytes_per_launch" in e:
            out.append(f"`{k.split('<')[0]}<{k.split('<')[1][:14]}` {e['hbm_bytes_per_launch'] / 1e9:.2f} GB per launch")
    return "; ".join(out[:3]) or "(see file)"


def sq(path):
    j = _load(path) or {}
    out = []
    for k, c in j.items():
        if "composite" in k and "GRBM_GUI_ACTIVE" in c and "SQ_ACTIVE_INST_VALU" in c:
            cyc = c["GRBM_GUI_ACTIVE"] / 8.0
            out.append(f"`{k[:34]}` VALU-busy {c['SQ_ACTIVE_INST_VALU'] * 4 / (1024 * cyc):.2f}, "
                       f"{(c.get('SQ_INSTS_VALU', 0) - c.get('SQ_INSTS_MFMA', 0)) / 1e6:.0f} M VALU + {c.get('SQ_INSTS_MFMA', 0) / 1e6:.0f} M MFMA wave-instr per launch")
    return "; ".join(out[:2]) or "(see file)"


def timeline(path):
    last = [ln for ln in open(path) if "span" in ln]
    return last[-1].strip() if last else "(see file)"


def bench(path):
    j = _load(path)
    if not isinstance(j, dict) or "value" not in j:
        return "(see file)"
    s = f"{j['value']} {j.get('unit', '')}, {j.get('ms_per_step')} ms per step"
    if isinstance(j.get("repeats"), dict):
        s += f" (median of {j['repeats']['regions']} regions: {j['repeats']['frames_per_s_min']} – {j['repeats']['frames_per_s_max']})"
    r = j.get("roofline")
    if isinstance(r, dict) and r.get("avg_ms"):
        s += f"; dominant kernel `{r.get('kernel')}` {r['avg_ms']} ms per launch = {r.get('achieved')} GB/s = {r.get('frac')} of the HBM peak"
    wl = (j.get("config") or {}).get("workload", "")
    return s + (f" — {wl[:90]}" if wl else "")


def clocks(path):
    j = _load(path) or {}
    a = j.get("amdsmi_library_20hz") or {}
    c, p = a.get("gfxclk_mhz_mean_over_xcds") or {}, a.get("socket_power_w") or {}
    res = (a.get("residency_counters_first_last") or {})
    acc, ppt = res.get("accumulation_counter"), res.get("ppt_residency_acc")
    frac = f", power-limit (PPT) residency {100 * (ppt[1] - ppt[0]) / max(acc[1] - acc[0], 1):.0f} % of the samples' time" if acc and ppt else ""
    return (f"gfx clock mean over the 8 XCDs {c.get('median')} MHz median ({c.get('min')} – {c.get('max')}), socket power {p.get('median')} W median "
            f"of a {j.get('power_cap_w')} W cap{frac}, {a.get('samples')} samples at {a.get('sample_rate_hz')} Hz, bench {j.get('bench_value_frames_per_s')} frames/s")


def gradbars(path):
    j = _load(path) or {}
    out = []
    for c in j.get("cases", []):
        if c["rtol"] == 1e-4 and c["oracle_alpha_mode"] == 0:
            t = c["tensors"]["dL_dmeans3D"]
            out.append(f"{c['workload']} {'accurate' if c['deterministic'] else 'normal'} mode: dL/dmeans3D needs <= {t['by_tensor_max_q'][-1]:.1e} of the tensor max, "
                       f"{t['row_frac_above']['0.001']:.1e} of its elements > 1e-3 of their row max")
    return "; ".join(out) or "(see file)"


def idle(path):
    j = _load(path) or {}
    return (f"{j.get('workload')}: wall {j.get('wall_us_per_iteration')} us / iteration, GPU busy {j.get('gpu_busy_us_per_iteration_torch_profiler')} us, "
            f"idle {j.get('idle_us_per_iteration')} us, host enqueue {j.get('host_enqueue_us_per_iteration')} us")


def scenelists(path):
    j = _load(path) or {}
    top = ", ".join(f"{k['kernel'].split('(')[0].replace('void sr::', '').replace('sr::', '')[:28]} {k['us']}" for k in (j.get("kernels") or [])[:3]
                    if isinstance(k, dict) and "kernel" in k and "us" in k)
    return (f"{j.get('keyframes')} key-frames, {j.get('rows')} rows, front end {j.get('front_end')}: refinement {j.get('refine_us_per_iteration')} us / iteration"
            + (f"; largest kernels (us): {top}" if top else ""))


def scene(path):
    j = _load(path) or {}
    if "map_ms_per_iteration" not in j:
        return ""
    return (f"; map {j['map_ms_per_iteration']} ms / iteration, refinement {j.get('refine_ms_per_iteration')} ms / iteration, "
            f"{j.get('rows_final')} rows, peak {j.get('peak_memory_GB')} GB")


def ab(path):
    j = _load(path) or {}
    out = []
    for n, v in (j.get("variants") or {}).items():
        s_ = f"{n} {v['fps']['mean']:.1f} frames/s"
        d = (j.get("vs_base") or {}).get(n)
        if d:
            f = d["fps_diff"]
            s_ += f" ({f['mean']:+.2f}, CI {f['ci95'][0]:+.2f} .. {f['ci95'][1]:+.2f}{', significant' if f.get('significant_at_5pct') else ''})"
        if "sclk_mhz" in v:
            s_ += f" at {v['sclk_mhz']['mean']:.0f} MHz / {v['power_w']['mean']:.0f} W"
        out.append(s_)
    return f"{j.get('workload')}, {j.get('runs_per_variant')} runs per variant: " + "; ".join(out) if out else "(see file)"


def perview(path):
    j = _load(path) or {}
    keys = [k for k in j if isinstance(j[k], (int, float)) and ("us" in k or "ms" in k)][:6]
    return ", ".join(f"{k} {j[k]}" for k in keys) or "(see file)"


def mapidle(path):
    j = _load(path) or {}
    return (f"{j.get('workload')}, densify every {j.get('densify_every')}: wall {j.get('wall_us_per_step')} us / step, GPU busy "
            f"{j.get('gpu_busy_us_per_step_torch_profiler')} us (raster {j.get('raster_kernels_us_per_step')}, other {j.get('non_raster_kernels_us_per_step')}), "
            f"idle {j.get('idle_us_per_step')} us, {j.get('kernels_per_step')} kernels")


def rccl(path):
    j = _load(path) or {}
    return f"backend {j.get('backend')}, RCCL {j.get('rccl_version')}, HSA_ENABLE_IPC_MODE_LEGACY={((j.get('env') or {}).get('HSA_ENABLE_IPC_MODE_LEGACY'))}, ok = {j.get('ok')}"


def landmark(path):
    j = _load(path) or {}
    rows = j.get("rows") or []
    if not rows:
        return "(no rows)"
    sc = [r["scores_ms"] for r in rows]
    se = [r["select_ms"] for r in rows]
    return (f"{j.get('visible_pairs', '?')} visible (point, view) pairs; scores {min(sc):.2f}-{max(sc):.2f} ms, sort + greedy pick "
            f"{min(se):.0f}-{max(se):.0f} ms ({rows[0].get('passes', '?')} passes) over {len(rows)} runs")


def matching(path):
    j = _load(path) or {}
    rows = j.get("rows") or []
    if not rows:
        return "(no rows)"
    parts = [f"({r['N1']}, {r['N2']}) {min(r['cost_plus_solve_ms']):.1f} ms vs CPU {r['cpu_matmul_ms'] + r['cpu_scipy_ms']:.0f} ms"
             for r in rows]
    b = j.get("batch") or {}
    c = j.get("candidates") or {}
    return (", ".join(parts) + f"; B = {b.get('B', '?')} batch {b.get('problems_per_s', '?')} problems/s; candidates "
            f"{min(c.get('ms') or [0]):.2f} ms")


def pnp(path):
    j = _load(path) or {}
    rows = j.get("rows") or []
    if not rows:
        return "(no rows)"
    parts = [f"N = {r['N']} at {r['outlier_share']} outliers {min(r['ms']):.2f} ms" for r in rows]
    b = j.get("batch") or {}
    return ", ".join(parts) + f"; B = {b.get('B', '?')} batch {min(b.get('ms') or [0]):.1f} ms"


def localize(path):
    j = _load(path) or {}
    rows = j.get("retrieval") or []
    d = j.get("driver") or {}
    if not rows or not d:
        return "(no rows)"
    parts = [f"Q = {r['Q']}, N = {r['N']}, D = {r['D']}, k = {r['k']}: {r['retrieve_ms']:.3f} ms vs torch {r['torch_einsum_topk_ms']:.3f} ms "
             f"(workspace {r['workspace_bytes'] / 1e6:.2f} MB, matrix {r['similarity_matrix_bytes'] / 1e6:.1f} MB)" for r in rows]
    return ("; ".join(parts) + f"; {d['queries']} queries on {d['frames']} frames: localize {d['localize_ms']:.0f} ms vs per-query loop "
            f"{d['per_query_loop_ms']:.0f} ms ({d['ratio_loop_over_localize']:.2f} x), bit-identical {d['bit_identical_to_loop']}")


def imageops(path):
    j = _load(path) or {}
    if not j.get("rows"):
        return str(j.get("status", "not measured"))
    return "; ".join(f"{r['dataset_type']} {r['W']}x{r['H']} N = {r['N']}: {r['hip']['median_ms']:.4f} ({r['hip']['min_ms']:.4f} - {r['hip']['max_ms']:.4f}) "
                     f"vs {r['torch_operators']['median_ms']:.3f} ({r['torch_operators']['min_ms']:.3f} - {r['torch_operators']['max_ms']:.3f}), "
                     f"{r['pixels_that_differ']} pixels differ" for r in j["rows"])


def sphead(path):
    j = _load(path) or {}
    if not j.get("rows"):
        return str(j.get("status", "not measured"))
    out = []
    for r in j["rows"]:
        if r["what"] == "detect":
            out.append(f"{r['logits']} candidates B = {r['B']} ({min(r['candidates'])} - {max(r['candidates'])} per image): "
                       f"{r['hip_device']['median_ms']:.4f} [{r['hip_host']['median_ms']:.4f}] vs {r['torch_operators_device']['median_ms']:.3f} "
                       f"[{r['torch_operators_host']['median_ms']:.3f}]")
        else:
            out.append(f"dense B = {r['B']}, {r['rows']} rows: {r['hip_device']['median_ms']:.4f} for {r['bytes_written'] / 1e6:.0f} MB, "
                       f"{r['write_GBps']:.0f} GB/s = {r['fraction_of_hbm_peak']:.3f} of the HBM peak")
    return "; ".join(out)


def nvhead(path):
    j = _load(path) or {}
    if not j.get("rows"):
        return str(j.get("status", "not measured"))
    out = []
    for r in j["rows"]:
        if "hip" not in r:
            continue
        others = " / ".join(f"{r[k]['median_ms']:.4f}" for k in ("torch_operators", "torch_operators_literal", "torch_operators_gemm") if k in r)
        txt = f"{r['what']} B = {r['B']}: {r['hip']['median_ms']:.4f} vs {others}"
        if "byte_floor_ms" in r:
            txt += f" (byte floor {r['byte_floor_ms']:.4f}: {r['fraction_of_byte_floor']:.3f} of it)"
        out.append(txt)
    return "; ".join(out) + f"; project B = 8 over B = 1: {j['project_B8_over_B1']:.3f}"


def convnet(path):
    j = _load(path) or {}
    if not j.get("rows"):
        return str(j.get("status", "not measured"))
    out = []
    for r in j["rows"]:
        if r["what"] == "layer":
            continue
        out.append(f"{r['what']} B = {r['B']}: {r['hip']['median_ms']:.4f} vs {r['torch_conv2d']['median_ms']:.4f} (floor {r['mfma_floor_ms']:.4f}: "
                   f"{r['fraction_of_floor']:.3f} of it)")
    layers = [r for r in j["rows"] if r["what"] == "layer"]
    if layers:
        fr = [r["fraction_of_floor"] for r in layers]
        ro = [r["hip_over_torch"] for r in layers]
        out.append(f"{len(layers)} layer rows: fraction of the floor {min(fr):.3f} - {max(fr):.3f}, time over torch's {min(ro):.3f} - {max(ro):.3f}")
    return "; ".join(out)


def jointwindow(path):
    j = _load(path) or {}
    if not j.get("results"):
        return str(j.get("status", "(no rows)"))
    parts = []
    for r in j["results"]:
        v = r["variants"]
        parts.append(f"{r['workload']} ({r['width']}x{r['height']}, C = {r['channels']}, P = {r['P']}): joint call {v['joint']['ms_per_window_backward']:.4f} "
                     f"({v['joint']['min']:.4f} - {v['joint']['max']:.4f}), `window_backward` + `window_backward_cameras` "
                     f"{v['two_calls']['ms_per_window_backward']:.4f} ({v['two_calls']['this_over_joint']:.3f} x), five per-view calls "
                     f"{v['per_view']['ms_per_window_backward']:.4f} ({v['per_view']['this_over_joint']:.3f} x)")
    return "; ".join(parts)


def refinebounded(path):
    j = _load(path) or {}
    if not j.get("shapes"):
        return str(j.get("status", "(no rows)"))
    parts = []
    for r in j["shapes"]:
        d = r["paired_plain_minus_bounded_us"]
        parts.append(f"{r['shape']} (P = {r['P']}): plain {r['plain']['wall_us_per_iteration']:.1f} wall / {r['plain']['host_enqueue_us_per_iteration']:.1f} host / "
                     f"{r['plain']['kernel_us_per_iteration_torch_profiler']:.1f} kernels, bounded {r['bounded']['wall_us_per_iteration']:.1f} / "
                     f"{r['bounded']['host_enqueue_us_per_iteration']:.1f} / {r['bounded']['kernel_us_per_iteration_torch_profiler']:.1f}; paired plain - bounded "
                     f"{d['mean']:+.1f} us (2 s.e. {d['two_standard_errors']:.1f}), faster beyond the spread: {r['bounded_faster_beyond_paired_spread']}, "
                     f"rewinds {r['rewinds_in_timed_regions']}")
    return "; ".join(parts)


def posewindow(path):
    j = _load(path) or {}
    if not j.get("results"):
        return str(j.get("status", "(no rows)"))
    parts = []
    for r in j["results"]:
        v = r["variants"]
        wins = ", ".join(f"window {k.split('_')[1]} {v[k]['ms_per_frame_iteration']:.4f}" for k in v if k != "loop")
        parts.append(f"{r['workload']} (P = {r['P']}): loop {v['loop']['ms_per_frame_iteration']:.4f} ({v['loop']['min']:.4f} - {v['loop']['max']:.4f}), "
                     f"{wins}; best window {r['best_window']} ({v['window_%d' % r['best_window']]['loop_over_this']:.3f} x the loop's speed), "
                     f"poses within 2e-4 of the loop's: {r['poses_agree_within_2e-4']}")
    return "; ".join(parts)


def decoder(path):
    j = _load(path) or {}
    names = (("train_step_batch_256", "training step at batch 256"), ("inference_5000", "inference at N = 5 000"),
             ("inference_1000000", "inference at N = 1 000 000"))
    parts = [f"{label} {j[k]['fused_ms']:.3f} vs {j[k]['composed_ms']:.3f} ms" for k, label in names if k in j]
    if not parts:
        return "(no rows)"
    tf = (j.get("inference_1000000") or {}).get("fused_TFLOPS")
    return ", ".join(parts) + (f" ({tf} TFLOPS)" if tf is not None else "")


def fusionmesh(path):
    j = _load(path) or {}
    ms, tb = j.get("ms") or {}, j.get("achieved_TB_per_s") or {}
    if not ms:
        return "(no rows)"
    return (f"{j.get('vertices')} vertices, {j.get('faces')} faces; surface() {ms['surface']:.2f} ms, count + scan {ms['mesh_count']:.2f} "
            f"({tb.get('mesh_count')} TB/s), faces {ms['mesh_faces']:.2f} ({tb.get('mesh_faces')} TB/s), normals {ms['mesh_normals']:.2f} "
            f"({tb.get('mesh_normals')} TB/s); the copy {j.get('measured_copy_TB_per_s')} TB/s")


def fusion(path):
    j = _load(path) or {}
    ms, tb = j.get("ms_per_frame") or {}, j.get("achieved_TB_per_s") or {}
    if not ms:
        return "(no rows)"
    return (f"single frames {ms['single']:.2f} ms per frame ({tb.get('single')} TB/s), batches of 8 {ms['batch8']:.2f} ({tb.get('batch8')} TB/s), "
            f"torch composition {ms['torch']:.1f}")


def setup_pmc(path):
    j = _load(path) or {}
    return "; ".join(f"{c} {j['parent'][c] / 1e6:.1f} M -> {j['change'][c] / 1e6:.1f} M ({j['delta_per_wave'][c]:+.0f} per wave)"
                     for c in ("SQ_INSTS_SALU", "SQ_INSTS_VALU"))


def kstats2(path):
    rows = [ln.split() for ln in open(path) if ln.startswith("composite_bwd_kernel<35")]
    return "`composite_bwd_kernel<35>` " + " -> ".join(f"{float(r[-6]):.2f}" for r in rows) + " us avg"


def setup_ab(path):
    c = (_load(path) or {})["change_vs_parent"]
    k = c["bwd_kcycles_ms_x_mhz"]
    return (f"change minus parent {c['fps_diff_pct_of_parent_mean']['mean']:+.2f} % of the parent's frames/s (CI "
            f"{c['fps_diff_pct_of_parent_mean']['ci95'][0]:+.2f} .. {c['fps_diff_pct_of_parent_mean']['ci95'][1]:+.2f} %), backward "
            f"{c['bwd_ms']['parent']:.4f} -> {c['bwd_ms']['change']:.4f} ms, ms x MHz {k['parent']['mean']:.0f} -> {k['change']['mean']:.0f}")


def pc_kstats(path):
    halves, out = open(path).read().split("# rocprofv3")[1:], []
    for name in ("payload_kernel", "ranges_kernel", "payload_tile_kernel", "composite_fwd_kernel<35>", "composite_bwd_kernel<35"):
        per = []
        for h in halves:
            rows = [ln.split() for ln in h.splitlines() if ln.startswith(name)]
            per.append(" + ".join(f"{float(r[-6]):.1f}" for r in rows) or "-")
        out.append(f"`{name}` " + " -> ".join(per))
    return "; ".join(out)


def pc_pmc(path):
    j = _load(path) or {}
    w = j.get("written_MB_per_launch") or {}
    return (f"live fraction {j.get('live_fraction', {}).get('live_fraction')}; MB written per launch (WRITE_SIZE as reported): "
            + ", ".join(f"{k} {v:.0f}" for k, v in w.items()))


def pc_ab(path):
    c = (_load(path) or {}).get("change_vs_parent")
    if not c:
        return "(other workload: frames/s only)"
    return (f"change minus parent {c['fps_diff_pct_of_parent_mean']['mean']:+.2f} % of the parent's frames/s (CI "
            f"{c['fps_diff_pct_of_parent_mean']['ci95'][0]:+.2f} .. {c['fps_diff_pct_of_parent_mean']['ci95'][1]:+.2f} %, margin {c['margin_pct']} %); "
            + "; ".join(f"{k} {v['parent_ms']:.4f} -> {v['change_ms']:.4f} ms, ms x MHz {v['parent_kcycles']:.0f} -> {v['change_kcycles']:.0f}"
                        for k, v in c["stages"].items()))


def dm_share(path):
    j = _load(path) or {}
    return (f"{j['marked_dead_among_walked']} of the {j['walked_by_backward']} candidate-quadrants the backward walks are marked "
            f"({100.0 * j['share_of_walked']:.2f} %; the issue's CPU estimate: {100.0 * j['cpu_estimate_of_the_issue']:.1f} %)")


def dm_room(path):
    j = _load(path) or {}
    return f"{j['marked_dead_among_walked']} of {j['walked_by_backward']} walked candidate-quadrants ({100.0 * j['share_of_walked']:.2f} %), {j['rows']} rows, {j['keyframes']} key-frames"


def fe_kstats(path):
    """the two listings' large launches of the front-end kernels (the tile sort's; the depth sort's small ones share the names)"""
    halves, out = open(path).read().split("# rocprofv3")[1:], []
    for name in ("payload_kernel", "emit_kernel", "sort_hist_kernel", "sort_scatter_kernel"):
        per = []
        for h in halves:
            rows = [ln.split() for ln in h.splitlines() if ln.startswith(name)]
            per.append(" + ".join(f"{float(r[-6]):.1f}" for r in rows) or "-")
        out.append(f"`{name}` " + " -> ".join(per))
    return "; ".join(out)


def fe_pmc(path):
    j = _load(path) or {}
    f = j.get("payload_kernel_fetched_MB_per_launch") or {}
    return "`payload_kernel` fetched MB per launch (FETCH_SIZE as reported, not doubled): " + ", ".join(f"{k} {v:.0f}" for k, v in f.items())


def fe_ab(path):
    c = (_load(path) or {})["change_vs_parent"]
    return (f"change minus parent {c['fps_diff_pct_of_parent_mean']['mean']:+.2f} % of the parent's frames/s (CI "
            f"{c['fps_diff_pct_of_parent_mean']['ci95'][0]:+.2f} .. {c['fps_diff_pct_of_parent_mean']['ci95'][1]:+.2f} %, margin {c['margin_pct']} %), "
            f"tile-sort stage {c['tile_sort_ms']['parent']:.4f} -> {c['tile_sort_ms']['change']:.4f} ms, payload stage {c['payload_ms']['parent']:.4f} -> "
            f"{c['payload_ms']['change']:.4f} ms ({', '.join(f'{k} {v:.4f}' for k, v in c['payload_ms_of_band_variants'].items())})")


EXTRACT = {"dm_share": dm_share, "dm_room": dm_room, "pc_kstats": pc_kstats, "pc_pmc": pc_pmc, "pc_ab": pc_ab, "fe_kstats": fe_kstats, "fe_pmc": fe_pmc, "fe_ab": fe_ab, "setup_pmc": setup_pmc, "kstats2": kstats2, "setup_ab": setup_ab, "scenelists": scenelists, "scene": scene, "ab": ab, "perview": perview, "mapidle": mapidle, "rccl": rccl, "kstats": kstats, "hbm": hbm, "sq": sq, "timeline": timeline, "bench": bench, "clocks": clocks, "gradbars": gradbars, "idle": idle, "landmark": landmark, "matching": matching, "pnp": pnp, "decoder": decoder, "fusion": fusion, "fusionmesh": fusionmesh, "localize": localize, "imageops": imageops, "sphead": sphead, "nvhead": nvhead, "convnet": convnet, "jointwindow": jointwindow, "posewindow": posewindow, "refinebounded": refinebounded}


def describe(name, path):
    for pat, text in WHAT:
        if re.search(pat, name):
            for key, fn in EXTRACT.items():
                if "{" + key + "}" in text:
                    try:
                        text = text.replace("{" + key + "}", fn(path))
                    except Exception as ex:  # noqa: BLE001
                        text = text.replace("{" + key + "}", f"(unreadable: {ex!r})")
            return text
    return "(undescribed)"


def render() -> str:
    files = sorted((os.path.basename(p) for p in glob.glob(os.path.join(PROF, "*")) if not p.endswith("README.md")),
                   key=lambda n: (not n.startswith("r"), -(int(n[1:3]) if re.match(r"r\d\d_", n) else 0), n))
    lines = ["# profiles/ — rocprofv3 evidence, per round", "",
             "All numbers: MI355X (gfx950), `bench.py`.  **This table is generated** by `tools/profiles_readme.py` from the files it",
             "describes: every figure below is read out of the file in the same row.  Collected on the GPU box with",
             "`tools/gpu_profile.sh` / `tools/pmc_passes.sh` / `tools/clock_trace.py`, condensed by `tools/summarize_prof.py`, copied here by",
             "`tools/collect_profiles.py` (raw rocpd databases stay in the scratch directory `gpurun_out/`).", "",
             "| file | what |", "|---|---|"]
    for n in files:
        lines.append(f"| `{n}` | {describe(n, os.path.join(PROF, n))} |")
    return "\n".join(lines) + "\n"


def main():
    txt = render()
    with open(os.path.join(PROF, "README.md"), "w") as f:
        f.write(txt)
    print("wrote profiles/README.md:", txt.count("\n| `"), "files;", txt.count("(undescribed)"), "undescribed")


if __name__ == "__main__":
    main()
