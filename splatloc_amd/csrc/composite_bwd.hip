// composite_bwd.hip — backward of the alpha compositing (SURVEY.md §8a "COMPOSITE bwd").
//
// Replaces the render-backward stage of the rasterizer extension whose backward is
// triggered at train_gaussians.py:229 / :286.
//
// Formulation (round 4: BACK-TO-FRONT, the lineage's direction; rounds 1-3 walked front to back): with
// q_i = f_i . g + z_i g_D (g = dL/dcolor at the pixel), T_i the transmittance in front of Gaussian i and
//     A_i = [ sum_{j>i} alpha_j T_j q_j + T_final (bg . g - g_A) ] / T_{i+1}      (what lies behind i, per unit of light reaching it)
// the derivative is  dL/dalpha_i = T_i (q_i - A_i)  and the state moves towards the camera by
//     T_i = T_{i+1} / (1 - alpha_i),     A_{i-1} = A_i + alpha_i (q_i - A_i),
// started at every pixel's last contributor with T = final_T and A = bg . g - g_A (exact).  One dot product per (pixel, Gaussian),
// linear in (g, g_D, g_A) — channels can be split over several launches (generic C).  Every quantity is O(1)-scaled: errors stay
// RELATIVE to the Gaussian's own gradient.  The front-to-back form of rounds 1-3, S_i = S_total - sum_{j<=i} w_j q_j with S_total =
// out_color . g, carried an ABSOLUTE error of ~1e-7 |S_total| in float32 that was up to 1e-3 of the S_i of a Gaussian behind
// T = 1e-4 (profiles/r04_grad_bars_before_accurate_mode.json); it also needed the forward's C + 1 colour / depth planes, which
// this form does not read (except at the boundaries of split launches, below).  alpha itself is evaluated with the forward's
// arithmetic (composite_common.h), and which entries contribute is the forward's decision (n_contrib), so the two passes agree
// on every alpha >= 1/255 / T < 1e-4 test.
//
// Machine mapping = the forward's (composite_fwd.hip): ONE wave64 = one workgroup = one 8x8
// quadrant, the tile's list streamed from the per-instance payload (mask byte + record),
// candidates' feature rows gathered into LDS, candidates processed two at a time; no
// __syncthreads.  Per (wave, Gaussian) the per-pixel partials are summed over the 64 pixels:
//   * 7 geometric partials (+ channels beyond the first 32) of BOTH Gaussians of a pair:
//     one packed butterfly reduction (permlane32/16 swap + DPP, ~2.2 VALU per value) and one
//     wave-wide float atomic;
//   * NC >= 32: dL/dfeature[g][ch] = sum_pix w[pix][g] * dL/dcolor[pix][ch] for the first 32
//     channels is a dense [16 g x 64 pix] x [64 pix x 32 ch] contraction per group of 16
//     contributing Gaussians: the weights are parked in a 4-KB LDS panel (one ds_write per
//     step), the dL/dcolor panel lives in registers for the whole tile, and the contraction
//     runs on the matrix pipe with v_mfma_f32_16x16x4_f32 — exact fp32 (k-ordered fmaf chain).
#include <type_traits>

#include "composite_common.h"

#ifndef SR_BWD_FS
#define SR_BWD_FS 32  // feature rows staged per round (<= 64)
#endif
#ifndef SR_BWD_STAGE_UNROLL
#define SR_BWD_STAGE_UNROLL 3  // gather iterations in flight together while staging feature rows (A/B on S2, 5 cameras: 2: 0.947, 3: 0.914 ms)
#endif

#ifndef SR_BWD_MINW
#define SR_BWD_MINW 4  // waves per SIMD the register allocator must allow (A/B on S2: 1.035 vs 1.07 ms at 3)
#endif

#ifndef SR_BWD_DOT_CHAINS
#define SR_BWD_DOT_CHAINS 2  // (>= 1) independent accumulators of the 4x4x1 MFMA dot product (A/B: 1: 0.950, 2: 0.928, 3: 0.944 (other box), 6 spills)
#endif
#ifndef SR_BWD_SMALL_PANEL_MAX_WAVES
#define SR_BWD_SMALL_PANEL_MAX_WAVES 6144  // frames with at most this many quadrant-waves use the small-layout panel variant (0 = never)
#endif
#ifndef SR_BWD_DOT_PREFETCH
#define SR_BWD_DOT_PREFETCH 1  // double-buffered LDS reads in the 4x4x1 dot (A/B on S2: 0.8645 -> 0.860 ms)
#endif
// (The timing probes of rounds 2-3 that produce WRONG results by design — hot-row gathers, skipped staging, dropped atomics /
//  butterfly / MFMAs / plane loads — are not part of this translation unit: tools/patches/composite_probes.patch adds them
//  back for tools/ablate.py --patch.)
#ifndef SR_BWD_TM
#define SR_BWD_TM 1   // 1 = transposed moment reduction (small-layout panel variant): E = G dL/dalpha parked in an 8-column LDS panel, reduced by lane = (Gaussian, pixel column)
#endif
#ifndef SR_BWD_MINW_TM
#define SR_BWD_MINW_TM 3  // waves per SIMD of the NC >= 32 kernel WITH the E panel (12.6 KB of LDS per wave: 12 workgroups per CU)
#endif
#ifndef SR_BWD_DOTM_MIN
#define SR_BWD_DOTM_MIN 8  // channels from which the 4x4x1 MFMA dot product is used
#endif

namespace sr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int NC, bool SP, bool AUX = true>
struct BwdCfg {
    // Small layouts (NC <= 15: SplatLoc's own C = 4, and 1 / 2 / 3 / 8), variant SP: ALL channels and the depth
    // weight w g_D are ONE 16-column block of the flush contraction, so only the six geometric moments go
    // through the butterfly (12 instead of 22 values per pair at C = 4) — at the price of 91 instead of 59 VGPRs
    // (5 instead of 8 waves per SIMD).  It is chosen per launch: when the frame's quadrant-waves all fit the
    // machine at once anyway (SplatLoc's 640x480: 4 800 waves) the lost occupancy costs nothing and the kernel
    // is 8 % faster (C = 4: 0.252 -> 0.231 ms); on large frames the butterfly variant at full occupancy wins
    // (S1, 1200x680: 0.198 vs 0.238 ms), and below 4 channels the flush costs what it saves.
    static constexpr bool SMALLP = NC <= 15 && SP;
    static constexpr bool MFMA = NC >= 32 || SMALLP;
    // NC >= 32: channels 0-31 are the TWO 16-column blocks of the flush (NB = 2); the channels beyond 32 and the depth
    // weight are butterfly values (NV, KV below)
    static constexpr int NM = NC >= 32 ? 32 : (SMALLP ? NC : 0);   // channels reduced on the matrix pipe
    static constexpr int NB = NC >= 32 ? 2 : 1;         // 16-column blocks of the contraction
    static constexpr bool XD = SMALLP && AUX;              // column NC of the blocks = the depth weight
    static constexpr int NV = NC - NM;         // channels reduced with the packed butterfly
    // TM (small-layout panel variant; measured on the reference layout, 5 views: 0.791 -> 0.762 ms): the six geometric
    // moments leave the butterfly too.  E = G dL/dalpha is parked in an
    // 8-column LDS panel [64 pix][8 Gaussians]; every 8 Gaussians lane (g = l & 7, i = l >> 3) sums its Gaussian over
    // pixel column i (8 reads), forms the moments with ITS Gaussian's mean, and three swap stages fold the 8 columns:
    // ~8 VALU per Gaussian instead of 6 moment products + 13 butterfly instructions.
    static constexpr bool TM = SR_BWD_TM && SMALLP;
    static constexpr int EG = 8;               // Gaussians per E-panel reduction
    static constexpr int ES = 9;               // LDS row stride of the E panel [64 pix][EG]
    // AUX = false: no view of the launch has a depth / alpha gradient (color_refinement, train_gaussians.py:283-285):
    // the depth weight w g_D is identically zero and leaves the reduction
    static constexpr int KV = NV + ((XD || !AUX) ? 0 : 1) + (TM ? 0 : 6);   // butterfly values per Gaussian
    static constexpr int NCP = (NC + 3) & ~3;
    static constexpr int FS = SR_BWD_FS;             // feature rows staged per round
    static constexpr int GROUP = 16;           // Gaussians per MFMA flush (M of v_mfma_f32_16x16x4_f32)
    static constexpr int WS = 17;              // LDS row stride of the weight panel [64 pix][GROUP]
};

// Gradient accumulation.  Normal mode: float atomics (memory-side adds; the order in which the quadrant-waves
// of different tiles reach a Gaussian's row varies from run to run, so sums differ in the last bits).
// DET (splatraster_debug_set_deterministic — the reproducible AND accurate debug mode): every wave-level partial — itself
// computed in a fixed order — is converted to fixed point and added with a 64-bit INTEGER atomic: integer addition is
// associative, so the totals are bit-reproducible whatever the arrival order.  Round 4: the fixed point is chosen PER
// ELEMENT from the largest partial that element receives (round 3 used 2^-40 for everything: a resolution of 9e-13,
// which is 1e-3 of a gradient of 1e-9 — with mean-reduced losses, dL/dout ~ 1 / (H W), most rows of a 500k-Gaussian
// scene are that small).  The kernel therefore runs TWICE in this mode:
//   det_pass 0: atomicMax of the bit pattern of |partial| into the (zeroed) float accumulator — max is associative too;
//   det_pass 1: partial * 2^(170 - det_drop - biased exponent of that max) added as int64.  det_drop = 0 (one row per (view,
//               Gaussian)): |partial| * scale < 2^44, and up to 2^18 partials per element (4 quadrant-waves per tile a Gaussian
//               touches) cannot overflow 2^62; the resolution is 2^-44 of the element's LARGEST partial — twenty bits below a
//               float's.  det_drop = 3 (C >= 32, V > 1: an element of the shared colour table receives the partials of all V <= 8
//               views, up to 2^21): |partial| * scale < 2^41, the same 2^62 bound, resolution 2^-41 (common.h:
//               gacc_det_headroom_drop; the whole launch uses it, per-view rows included);
//   fixed_to_float_kernel (preprocess_bwd.hip) reads the same exponent and converts back.
constexpr int DET_HEADROOM_EXP = 170;   // scale exponent = DET_HEADROOM_EXP - biased exponent of max |partial|
__device__ __forceinline__ int det_scale_exp(unsigned max_bits)
{
    const int eb = (int)((max_bits >> 23) & 0xffu);
    return DET_HEADROOM_EXP - (eb > 0 ? eb : 1);
}
template <bool DET>
__device__ __forceinline__ void acc_add(float* gacc, long long* gacc64, size_t idx, float v, int det_pass, int det_drop)
{
    if (DET) {
        if (det_pass == 0) {
            atomicMax(reinterpret_cast<unsigned*>(gacc) + idx, __float_as_uint(fabsf(v)));
        } else {
            const unsigned mb = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(gacc) + idx);
            if (((mb >> 23) & 0xffu) == 0xffu) {
                // a NaN or an infinity reached this element (it won pass 0's maximum): no fixed point can hold it.  The element
                // must come back non-finite, like the float atomics of the normal path would leave it — this mode exists to
                // expose such failures, not to flush them to 0 (round-4 advisor finding).  NaN: the recorded maximum says it
                // all; infinities: their signs are counted (low word +inf, high word -inf) for fixed_to_float_kernel
                if (__builtin_isinf(v)) atomicAdd(reinterpret_cast<unsigned long long*>(gacc64) + idx, v > 0.f ? 1ull : (1ull << 32));
                return;
            }
            const double scaled = ldexp((double)v, det_scale_exp(mb) - det_drop);
            atomicAdd(reinterpret_cast<unsigned long long*>(gacc64) + idx, (unsigned long long)__double2ll_rn(scaled));
        }
    } else {
        (void)det_pass;
        (void)det_drop;
        atomicAdd(gacc + idx, v);
    }
}

// One step of the back-to-front walk (header): the state T, A behind an entry moves in front of it; out come dA = T_i (q_i - A_i)
// — dL/dalpha_i, finite also for a miss, where E = G dA = 0 — and the blending weight w = alpha_i T_i.  Branch-free: a miss keeps T
// and A and has w = 0.  ST = double in the accurate mode (DET), else float: there T_i = T_{i+1} / (1 - alpha) goes through the
// hardware reciprocal (1 ulp; alpha <= 0.99 keeps the argument >= 0.01) — a relative error per step, harmless; the correctly
// rounded division would be 10 instructions per Gaussian.
__device__ __forceinline__ float walk_divide(float T, float one_minus_alpha) { return T * __builtin_amdgcn_rcpf(one_minus_alpha); }
__device__ __forceinline__ double walk_divide(double T, double one_minus_alpha) { return T / one_minus_alpha; }
__device__ __forceinline__ float walk_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double walk_fma(double a, double b, double c) { return fma(a, b, c); }
template <typename ST>
__device__ __forceinline__ void walk_entry(ST& T, ST& A, bool hit, float alpha, float q, float& dA, float& w)
{
    const ST Ti = hit ? walk_divide(T, (ST)1 - (ST)alpha) : T;
    const ST d = (ST)q - A;
    dA = (float)(Ti * d);
    const ST ah = hit ? (ST)alpha : (ST)0;
    A = walk_fma(ah, d, A);
    w = (float)(ah * Ti);
    T = Ti;
}

// Where a wave adds its partials: the accumulator (GaccLayout, common.h) as the compositing kernel addresses it — column col of
// Gaussian id (its index in the view; < 2^24, checked on the host) at  mul24(id, stride) + offset,  stride and offset those of the
// table the column lives in.  A caller that knows the table at compile time names it and nothing is selected per pair: a kernel of
// NC >= 32 channels only exists for c0 + 32 <= C, so its flush columns [c0, c0 + 32) all lie in the SHARED table and its butterfly
// values (channels c0 + 32 .., moments) in the per-VIEW one; the moments are per view in every layout.  The narrower kernels serve
// any column range (the chunked passes of C = 40, 48 ...; C < 32: everything per view): BY_COLUMN.
enum class GaccTable { SHARED, VIEW, BY_COLUMN };
template <bool DET>
struct GradRows {
    float* __restrict__ gacc;
    long long* __restrict__ gacc64;
    GaccLayout GL;
    uint32_t row0, pv_base;   // the view's first row; GL.view_base24(row0)
    int det_pass, det_drop;
    __device__ __forceinline__ uint32_t stride(uint32_t col, GaccTable tb) const
    {
        return tb == GaccTable::SHARED ? GL.SH : (tb == GaccTable::VIEW ? GL.PV : GL.stride24(col));
    }
    __device__ __forceinline__ uint32_t offset(uint32_t col, GaccTable tb) const
    {
        return (tb == GaccTable::SHARED ? 0u : (tb == GaccTable::VIEW ? pv_base : GL.base24(col, row0))) + col;
    }
    // (stride and offset apart: where the column does not change from pair to pair they are hoisted out of the loops)
    static __device__ __forceinline__ size_t index(uint32_t id, uint32_t stride, uint32_t offset) { return (size_t)(__umul24(id, stride) + offset); }
    __device__ __forceinline__ size_t index(uint32_t id, uint32_t col, GaccTable tb) const { return index(id, stride(col, tb), offset(col, tb)); }
    __device__ __forceinline__ void add(size_t idx, float v) const { acc_add<DET>(gacc, gacc64, idx, v, det_pass, det_drop); }
};

template <int NC, bool SP, bool AUX>
constexpr int bwd_min_waves() { return (BwdCfg<NC, SP, AUX>::TM && NC >= 32) ? SR_BWD_MINW_TM : SR_BWD_MINW; }

template <int NC, bool DET, bool SP, bool AUX>
__global__ void __launch_bounds__(WAVE, (bwd_min_waves<NC, SP, AUX>()))
composite_bwd_kernel(int W, int H, int C_total, int CP4, int c0, int first_pass, int tiles /*per view*/, int V,
                     int P /*rows per view*/,
                     const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ ipack /*id | reach bits << 24*/,
                     const float4* __restrict__ irec, const float4* __restrict__ featp4,
                     WinGrad grads,
                     const float* __restrict__ final_T_all, const uint32_t* __restrict__ n_contrib_all,
                     float* __restrict__ gacc /*GaccLayout (common.h)*/, GaccLayout GL,
                     int MO /*column of the moments*/, long long* __restrict__ gacc64 /*same layout, fixed point, DET only*/,
                     const float* __restrict__ ckpt_all /*split launches (common.h; gridDim.y == SPLIT_PARTS): the forward's segment
                                                          records (segment_record), else null*/,
                     const uint32_t* __restrict__ nparts /*split launches: parts of every (view, tile) list, or null: SPLIT_PARTS*/,
                     int extra_blocks /*split launches: workgroups at the head of the grid that walk parts 4 .. of the longest lists*/,
                     const uint32_t* __restrict__ tile_order /*launch order (binning.hip), or null*/,
                     int det_pass /*DET only: 0 = per-element max of |partial|, 1 = fixed-point sums (acc_add)*/,
                     uint32_t cand_bits /*quadrant 0's bits of a list word that decide a candidate: IPACK_REACH0 | IPACK_DEAD0, or
                                          IPACK_REACH0 alone (the forward's dead marks ignored: splatraster_debug_set_dead_marks)*/)
{
    using Cfg = BwdCfg<NC, SP, AUX>;
    // DET (the accurate mode): the walk's state T, A and everything derived from it in double; else float
    using ST = typename std::conditional<DET, double, float>::type;
    constexpr int NCP = Cfg::NCP, NM = Cfg::NM, NV = Cfg::NV, KV = Cfg::KV, FS = Cfg::FS;
    constexpr int WS = Cfg::WS, GROUP = Cfg::GROUP;
    constexpr bool MFMA = Cfg::MFMA, XD = Cfg::XD;
    constexpr int NB = Cfg::NB;
    constexpr bool TM = Cfg::TM;
    constexpr int EG = Cfg::EG, ES = Cfg::ES;
    constexpr bool DOTM = NC >= SR_BWD_DOTM_MIN;  // dot products q = f . g on the matrix pipe
    constexpr int PPR = NCP / 4;  // 16-byte pieces per staged row
    static_assert(2 * KV <= WAVE, "at most 25 butterfly-reduced channels per pass");
    // records of the staged candidates only (row-indexed, like s_feat): with the 64-entry chunk
    // records here the workgroup needs 11.2 KB and only 14 fit a CU; at 10 KB all 16 (4 / SIMD) do
    // (+ 1: the second Gaussian of a pair is ALWAYS read from row r0 + 1 — adjacent rows share one address register —
    //  also when the round's last pair has no second member: that row is then stale, and the pair's second half is masked)
    __shared__ __attribute__((aligned(16))) float4 s_rec0[FS + 1];
    __shared__ __attribute__((aligned(16))) float4 s_rec1[FS + 1];
    __shared__ __attribute__((aligned(16))) float s_feat[(FS + (DOTM ? 0 : 1)) * NCP];   // (the MFMA dot product clamps its rows)
    __shared__ uint32_t s_cgid[FS + 1];
    __shared__ float s_w[MFMA ? WAVE * WS : 1];   // matrix-pipe weight panel w[64 pix][GROUP]
    __shared__ uint32_t s_gid[MFMA ? GROUP : 1];  // Gaussian id of every parked panel column
    __shared__ float s_e[TM ? WAVE * ES : 1];     // E panel [64 pix][EG]: column c belongs to weight-panel slot e0 + c
    __shared__ float2 s_emean[TM ? GROUP : 1];    // projected mean of every parked Gaussian

    int gtile, quad;   // global tile = view * tiles + tile: the grid covers the V views of the window
    const int gx = tile_columns(W);
    int seg_y = (int)blockIdx.y;      // split launches: the part of the list this wave walks
    if (NC <= 4 && (int)blockIdx.x < extra_blocks) {
        // EXTRA workgroups (first in the grid: their lists are the launch's longest): group e / (ids of SPLIT_EXTRA_TILES tiles) walks
        // parts 4 (group + 1) + blockIdx.y of the list at position r of the launch order — if that list has so many parts
        const unsigned per = quadrant_blocks(SPLIT_EXTRA_TILES, gx);
        const unsigned group = blockIdx.x / per;
        int r;
        quadrant_of_block(blockIdx.x - group * per, SPLIT_EXTRA_TILES, gx, r, quad);
        if (r >= SPLIT_EXTRA_TILES || r >= V * tiles) return;
        gtile = (int)tile_order[r];
        seg_y += SPLIT_PARTS * (int)(group + 1u);
        if (seg_y >= (int)nparts[gtile]) return;
    } else {
        quadrant_of_block(blockIdx.x - (NC <= 4 ? (unsigned)extra_blocks : 0u), V * tiles, gx, gtile, quad, tile_order);
        if (gtile >= V * tiles) return;
    }
    const int lane = threadIdx.x;
    const QuadFrame F = quadrant_frame(W, H, tiles, V, P, ranges, gtile, quad, lane);   // the forward's frame (composite_common.h)
    const int view = F.view;
    const uint32_t row0 = F.row0;   // the view's first row: feature rows (and the accumulator's shared colour rows) are per Gaussian
    const bool inside = F.inside;
    const size_t plane = F.plane, pix = F.pix;   // (pix: only lanes inside the image use it)
    constexpr bool WIDE = NC >= 32;   // (accumulator addressing: GradRows)
    const int det_drop = DET ? gacc_det_headroom_drop(C_total, V) : 0;   // fixed-point headroom of a shared table (acc_add, common.h)
    // what the WIDE shortcuts of GradRows rest on: the flush covers exactly the 32 columns [c0, c0 + 32) (c0 + 32 <= C, so <= SH for any
    // multiple-of-16 SH >= 32 reached in steps of 32 or with NC < 48), every butterfly column is >= c0 + 32 >= SH or a moment
    static_assert(!WIDE || (Cfg::NM == 32 && NC < 48), "a wide kernel's flush columns are the shared table's, its butterfly columns the per-view row's");
    // (the headline kernel, NC = 35, covers all of C = 35, or of C = 36 without its last channel: gacc_shared_floats = 32 and
    //  gacc_view_floats = 16 for both — constants here instead of two more scalars held through the loops; the launcher checks them)
    constexpr bool FIXED = NC == 35;
    static_assert(!FIXED || (gacc_shared_floats(NC) == 32 && gacc_view_floats(NC) == 16 && gacc_shared_floats(NC + 1) == 32 &&
                             gacc_view_floats(NC + 1) == 16), "the constants of the headline kernel");
    if constexpr (FIXED) { GL.SH = 32u; GL.PV = 16u; }
    const GradRows<DET> rows{gacc, gacc64, GL, row0, GL.view_base24(row0), det_pass, det_drop};
    constexpr GaccTable FLUSH_COLS = WIDE ? GaccTable::SHARED : GaccTable::BY_COLUMN, BUTTERFLY_COLS = WIDE ? GaccTable::VIEW : GaccTable::BY_COLUMN;
    const float* __restrict__ dL_dcolor = grads.dL_dcolor[view];
    const float* __restrict__ dL_ddepth = grads.dL_ddepth[view];
    const float* __restrict__ dL_dalpha = grads.dL_dalpha[view];
    const float* __restrict__ dL_dlast = grads.dL_dlast[view];
    const int gc = grads.gc;   // channel planes behind dL_dcolor; channel C - 1 reads dL_dlast when gc < C; channels between: no gradient
    const float* __restrict__ final_T = final_T_all + (size_t)view * H * W;
    const uint32_t* __restrict__ n_contrib = n_contrib_all + (size_t)view * H * W;
    const float fx = (float)F.px, fy = (float)F.py;
    uint32_t beg = F.beg, end0 = F.end;
    // split launches: wave blockIdx.y of the quadrant takes part blockIdx.y of the tile's list — the forward's partition (split_parts)
    const uint32_t list0 = beg;                                // list positions (n_contrib) count from the tile's first entry
    const bool split = !DET && NC <= 4 && ckpt_all != nullptr;   // (the accurate mode starts every list at its head)
    const int seg = split ? seg_y : 0;
    const SplitParts parts = split_parts(split, nparts, gtile, end0 - beg);
    const int np = parts.np;
    if (split) {
        take_part(parts, seg, beg, end0);
        if (beg >= end0) return;
    }
    // Leave early: this quadrant only needs the list up to its deepest contributor, and a quadrant without a list or
    // without a contributor (empty regions of real frames, quadrants outside the image) has nothing to add — it returns
    // here, before the set-up loads its NC + 3 planes.
    uint32_t last = inside ? n_contrib[pix] : 0u;
    uint32_t wave_last = last;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) wave_last = max(wave_last, (uint32_t)__shfl_xor((int)wave_last, d, WAVE));
    uint32_t end = min(end0, list0 + wave_last);
    // WIDE only: the value is wave-uniform after the reduction; said so, the list's end and the chunk counter derived from it
    // live in scalar registers, which keeps the headline kernel <35> inside its 128-VGPR budget (tests/test_codegen_budget.py)
    if constexpr (WIDE) end = (uint32_t)__builtin_amdgcn_readfirstlane((int)end);
    if (beg >= end) return;   // (split launches: nothing of this part contributes)
    // per-pixel constants
    float g[NC];
    // state of the back-to-front walk: T = transmittance BEHIND the entry about to be processed, A = what lies behind it per
    // unit of light (header).  At a pixel's last contributor: T = final_T, A = bg . g - g_A.
    ST A = 0;
    ST T = 1;
    float gD = 0.0f;
    if (inside) {
        // a split launch's segment that ends in FRONT of this pixel's last contributor starts from the boundary state rebuilt
        // from the forward's segment records (common.h): T_b, and A_b = (what the later segments contribute) / T_b
        const bool from_ckpt = split && seg < np - 1 && list0 + last > end0;
        float s_end = 0.0f;
        // planes [0, gc) behind dL_dcolor, the LAST channel's plane behind dL_dlast, nothing in between.  Which channel reads
        // what is the same for every wave of the launch, so it is decided ONCE per wave by scalar compares and the planes are
        // then walked with a pointer: a load and an add per channel.  (Until this form the source of every channel was selected
        // on its own — a 64-bit multiply, two selects and spilled conditions per channel: ~1 300 scalar instructions per wave
        // of the headline kernel)  The loads stay independent and in flight together: no branch BETWEEN them —
        // with a branch per channel the compiler waits for every second load before issuing the next (seen in the .s: 21 x
        // s_waitcnt vmcnt(0) between the plane loads, backward + 4 %).
        // The pixel's other values are requested first and branch-free as well (an absent plane reads final_T and drops the
        // value), so that they travel with the colour planes instead of one memory latency each behind them.
        const float Tf = final_T[pix];
        const bool has_gD = AUX && first_pass && dL_ddepth != nullptr, has_gA = AUX && first_pass && dL_dalpha != nullptr;
        float vD = 0.0f, vA = 0.0f;
        if constexpr (AUX) {
            vD = (has_gD ? dL_ddepth : final_T)[pix];
            vA = (has_gA ? dL_dalpha : final_T)[pix];
        }
        const int cb = FIXED ? 0 : c0;                           // (the launcher enforces c0 == 0 for the headline kernel)
        const int n_plain = min(max(gc - cb, 0), NC);            // channels [0, n_plain) of this pass have a plane behind dL_dcolor
        // channel C_total - 1 travels apart when gc < C_total.  The passes of a launch tile [0, C) (launch_composite_bwd), so
        // that channel is the LAST one of the pass that holds it
        const bool last_apart = gc < C_total && cb + NC == C_total && dL_dlast != nullptr;
        const float* const src0 = dL_dcolor + pix;               // plane 0: what a channel without a gradient reads (and drops)
        const float* src = src0 + (size_t)(n_plain > 0 ? cb : 0) * plane;
        if (n_plain >= NC - 1) {
            // every channel is plain (the per-view drop-in, the benchmark), or all but the pass's last one (split_last = True)
#pragma unroll
            for (int ch = 0; ch < NC - 1; ++ch) {
                g[ch] = *src;
                src += plane;
            }
            const bool own = n_plain == NC;
            const float v = *(own ? src : (last_apart ? dL_dlast + pix : src0));
            g[NC - 1] = (own || last_apart) ? v : 0.0f;
        } else {
            // a few leading planes, zeros, then perhaps the plane that travels apart (the map step's split_last = 3 at C = 35;
            // passes beyond gc): the walk stops at the last plain plane and the values behind it are dropped
#pragma unroll
            for (int ch = 0; ch < NC - 1; ++ch) {
                const float v = *src;
                g[ch] = ch < n_plain ? v : 0.0f;
                src += ch + 1 < n_plain ? plane : (size_t)0;
            }
            const float v = *(last_apart ? dL_dlast + pix : src0);
            g[NC - 1] = last_apart ? v : 0.0f;
        }
        {   // s_end = bg . g over the background's entries that fall into this pass, in channel order (a term the old
            // 35-way clamp-and-select form added for a channel beyond the background was fmaf(0, g, s) == s).  AFTER the plane
            // loads: a conditional scalar load between them serialised them (measured: backward + 6 % on S2)
            const int nb = grads.bg ? grads.bg_channels : 0;
            const float* __restrict__ bgp = grads.bg;
            if (nb <= 4) {   // RGB (+ 1) backgrounds: at most the pass's first four channels
#pragma unroll
                for (int ch = 0; ch < (NC < 4 ? NC : 4); ++ch)
                    if (cb + ch < nb) s_end = fmaf(bgp[cb + ch], g[ch], s_end);
            } else {
#pragma unroll
                for (int ch = 0; ch < NC; ++ch)
                    if (cb + ch < nb) s_end = fmaf(bgp[cb + ch], g[ch], s_end);
            }
        }
        if (AUX && first_pass) {
            gD = has_gD ? vD : 0.0f;
            s_end -= has_gA ? vA : 0.0f;
        }
        T = (ST)Tf;
        A = (ST)s_end;
        if constexpr (NC <= 4) {
            if (from_ckpt) {
                // later segments first (the smallest contributions), this boundary's neighbour last
                float sfx = Tf * s_end;
                for (int k = np - 1; k > seg; --k) {
                    const float* ck = segment_record(ckpt_all, F, C_total, k, 0);   // (T, the launch's C_total colours, the depth)
#pragma unroll
                    for (int ch = 0; ch < NC; ++ch) sfx = fmaf(ck[(size_t)(1 + c0 + ch) * plane], g[ch], sfx);
                    if (AUX) sfx = fmaf(ck[(size_t)(1 + C_total) * plane], gD, sfx);
                }
                const float Tb = *segment_record(ckpt_all, F, C_total, seg + 1, 0);
                T = (ST)Tb;
                A = (ST)(sfx / Tb);        // (T_b >= 1e-4: the pixel was still active at the boundary)
            }
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) g[ch] = 0.0f;
    }
    // B operand of the contraction, kept in registers for the whole tile: for k-step kk and
    // channel half t, lane l holds dL/dcolor[pix = 4 kk + (l >> 4)][ch = 16 t + (l & 15)].
    // Built once by transposing through the (still unused) weight panel.
    float gt[MFMA ? 16 : 1][NB];
    if (MFMA) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) {
                const int c = 16 * t + ch;
                s_w[lane * WS + ch] = c < NC ? g[c < NC ? c : 0] : ((XD && c == NC) ? gD : 0.0f);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) gt[kk][t] = s_w[(4 * kk + (lane >> 4)) * WS + (lane & 15)];
        }
        __builtin_amdgcn_wave_barrier();
    }

    // wave_reduce_pack leaves total k in lane bitreverse6(k); values [0, KV) belong to the first
    // Gaussian of a pair, [KV, 2 KV) to the second; inside a Gaussian: NV colours then 7 geometric
    const int slotv = (int)(__brev((unsigned)lane) >> 26);
    const bool slot_second = slotv >= KV;
    const int sv = slot_second ? slotv - KV : slotv;
    const bool slot_col = sv < NV;
    const bool slot_ok = slotv < 2 * KV;
    const uint32_t slot_colv = (uint32_t)(slot_col ? (c0 + NM + sv) : (TM ? MO + 6 : MO + sv - NV));  // column of the Gaussian's row
    const uint32_t slot_stride = rows.stride(slot_colv, BUTTERFLY_COLS), slot_off = rows.offset(slot_colv, BUTTERFLY_COLS);
    int nslot = 0;  // Gaussians parked in the weight panel (wave-uniform)
    int e0 = 0;     // weight-panel slot of the E panel's column 0 (wave-uniform)

    // dL/dfeature of the parked Gaussians: D[g][ch] = sum_pix W[pix][g] * G[pix][ch]
    // (v_mfma_f32_16x16x4_f32: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
    //  D[row = 4 (l >> 4) + reg][col = l & 15])
    auto flush_panel = [&](int count) {
        __builtin_amdgcn_wave_barrier();
        f32x4 D[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) D[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int row = (lane >> 4) * WS + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float a = s_w[4 * kk * WS + row];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                D[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, gt[kk][t], D[t], 0, 0, 0);
            }
        }
        // column c = 16 t + (l & 15): channel c0 + c below NM, the depth weight (moment slot 6, first pass only) at NM
        const int j0c = lane & 15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gs = 4 * (lane >> 4) + r;
            if (gs < count) {
                const uint32_t gid = s_gid[gs];
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    const int c = 16 * t + j0c;
                    const bool full = 16 * t + 16 <= NM;   // every column of the block is a channel
                    const bool col_ok = full || c < NM || (XD && c == NM && first_pass);
                    const uint32_t col = (full || c < NM) ? (uint32_t)(c0 + c) : (uint32_t)(MO + 6);
                    if (col_ok) rows.add(rows.index(gid, col, FLUSH_COLS), D[t][r]);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    // Moments of the parked E columns.  Lane (g = l & 7, i = l >> 3) owns Gaussian column g and pixel column i of the
    // quadrant: it reads E[pix = 8 j + i][g] for the 8 rows j, multiplies by ITS Gaussian's offsets d = mean - pixel
    // (dx is constant in the lane), and the first three stages of the packed butterfly (lane bits 5, 4, 3 = the pixel
    // column) fold the 8 columns: lane l ends with moment (l >> 5 & 1) + 2 (l >> 4 & 1) + 4 (l >> 3 & 1) of Gaussian g.
    auto reduce_e = [&](int count) {
        if constexpr (TM) {
            __builtin_amdgcn_wave_barrier();
            const int eg = lane & 7, ei = lane >> 3;
            const float2 mu = s_emean[min(e0 + eg, GROUP - 1)];
            const float dx = mu.x - (float)(F.qx + ei);
            const float dy0 = mu.y - (float)F.qy;
            float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // sum E, sum E dy, sum E dy^2 (then the six moments)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = s_e[(8 * j + ei) * ES + eg];
                const float dy = dy0 - (float)j;
                const float ey = e * dy;
                m[5] += e;
                m[1] += ey;
                m[4] = fmaf(ey, dy, m[4]);
            }
            m[0] = m[5] * dx;    // sum E dx
            m[2] = m[0] * dx;    // sum E dx^2
            m[3] = m[1] * dx;    // sum E dx dy
            const float outv = wave_reduce_hi3<6>(m, lane);
            const int vi = ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1) + 4 * ((lane >> 3) & 1);
            if (eg < count && vi < 6) {
                rows.add(rows.index(s_gid[e0 + eg], (uint32_t)(MO + vi), GaccTable::VIEW), outv);
            }
            __builtin_amdgcn_wave_barrier();
        }
    };

    // chunk in flight: the packed word (id | reach bits) of list entry base + lane — ONE register, so that the prefetch really stays in flight
    // while the current chunk is processed.  (Rounds 1-3 also prefetched the 32-byte record into eight registers; at 128 VGPRs
    // the compiler spilled them to scratch right behind the loads — `global_load ... s_waitcnt vmcnt(0) ... scratch_store` —
    // which exposed the whole memory latency once per chunk.  The records of the <= FS candidates are now loaded in the staging
    // round, together with their feature rows: one latency per round, as before, and only for this quadrant's candidates.)
    // (the word stays RAW — id | reach bits << 24: bit and id are extracted where they are consumed, one chunk later; extracting
    //  them here made the compiler wait for the load right behind the prefetch, an exposed memory latency per chunk)
    uint32_t pw = 0;
    auto fetch = [&](uint32_t base, uint32_t& w_) {
        w_ = 0u;
        if (base + (uint32_t)lane < end) w_ = ipack[base + (uint32_t)lane];
    };
    // The list is walked from the quadrant's deepest contributor towards the camera, 64 entries at a time (chunk k = entries
    // [beg + 64 k, beg + 64 k + 64)), the candidates of a chunk from the highest list position down.
    const uint64_t gt_mask = (lane == WAVE - 1) ? 0ull : (~0ull << (lane + 1));   // list positions behind this lane's
    const int nchunks = (int)((end - beg + (WAVE - 1)) / WAVE);
    fetch(beg + (uint32_t)(nchunks - 1) * WAVE, pw);

#pragma unroll 1
    for (int chunk = nchunks - 1; chunk >= 0; --chunk) {
        const uint32_t base = beg + (uint32_t)chunk * WAVE;
        // a candidate may reach this quadrant AND the forward did not find it dead there (no lane live: then no pixel has
        // `idx < last && pass`, the entry leaves T and A alone and adds zeros — DESIGN.md §6.2)
        const bool cur_reach = (pw & (cand_bits << quad)) == (IPACK_REACH0 << quad);
        uint64_t cand = __builtin_amdgcn_ballot_w64(cur_reach);
        const uint32_t cur_gid = (pw & 0xFFFFFFu) - row0;   // the Gaussian's index in its view: what the feature and accumulator rows are addressed with
        // the chunk in front: requested now, consumed after this one (the loop's last iteration requests nothing: the guard
        // is per lane, so there is no wave-uniform branch around the loads)
        fetch(chunk > 0 ? base - WAVE : 0xFFFFFF00u, pw);
        const uint32_t idx0 = base - list0;
#pragma unroll 1
        while (cand != 0) {
            // ---- stage the records and feature rows of the LAST <= FS candidates (row 0 = the deepest) ----
            const int ncand = min(FS, (int)__popcll(cand));
            const int rank = __popcll(cand & gt_mask);
            const bool mine = cur_reach && ((cand >> lane) & 1ull) && rank < FS;
            __builtin_amdgcn_wave_barrier();
            if (mine) s_cgid[rank] = cur_gid;
            float4 rec_a = make_float4(0.f, 0.f, 0.f, 0.f), rec_b = rec_a;
            if (mine) {
                const size_t j = (size_t)base + lane;
                rec_a = irec[2 * j];
                rec_b = irec[2 * j + 1];
            }
            __builtin_amdgcn_wave_barrier();
            // 16-byte pieces of the 16-byte-aligned padded rows
#pragma unroll SR_BWD_STAGE_UNROLL
            for (int e = lane; e < ncand * PPR; e += WAVE) {
                const int row = e / PPR, pc = e - row * PPR;
                reinterpret_cast<float4*>(s_feat)[e] = featp4[(size_t)(__umul24(s_cgid[row], (uint32_t)CP4) + (uint32_t)((c0 >> 2) + pc))];
            }
            if (mine) {
                s_rec0[rank] = rec_a;
                s_rec1[rank] = rec_b;
            }
            __builtin_amdgcn_wave_barrier();
            // One pair of candidates (list positions j0 > j1: the deeper one first; staged rows r0, r1); qm0 / qm1 are
            // their dot products when the matrix pipe already produced them.  What is done per entry is written once, for entry e
            // of the pair (the compiler unrolls the two-trip loops over e: the arrays are registers; the statements keep the order they
            // had when every line stood there twice — both loads, both offsets, ... — which the schedule of the pair loop follows).
            auto process_pair = [&](int j0, int j1, bool has1, int r0, int r1, float qm0, float qm1) {
                const int r[2] = {r0, r1};
                float4 p[2], q[2];
                float dx[2], dy[2];
                for (int e = 0; e < 2; ++e) p[e] = s_rec0[r[e]], q[e] = s_rec1[r[e]];
                for (int e = 0; e < 2; ++e) dx[e] = p[e].x - fx, dy[e] = p[e].y - fy;
                // alpha and its tests are the forward's (pair_alpha: a NaN from an overflowed power is a miss, which is why a miss
                // zeroes G below, not dL/dalpha); which entries contribute is the forward's decision too (last = n_contrib)
                const PairAlpha pa = pair_alpha(q[0], dx[0], dy[0], q[1], dx[1], dy[1]);
                const float al[2] = {pa.al0, pa.al1}, Gr[2] = {pa.G0, pa.G1};
                // (the flags stay scalars: as elements of an array they were materialised as bytes)
                auto contributes = [&](int je, bool pass) { return (idx0 + (uint32_t)je < last) && pass; };
                const bool hit0 = contributes(j0, pa.pass0), hit1 = has1 && contributes(j1, pa.pass1);
                const float G[2] = {hit0 ? Gr[0] : 0.0f, hit1 ? Gr[1] : 0.0f};
                // ---- dot products q = f . g (+ depth) of both Gaussians ----
                float qd[2] = {qm0, qm1};
                if (!DOTM) {
                    for (int e = 0; e < 2; ++e) qd[e] = AUX ? p[e].z * gD : 0.0f;
#pragma unroll
                    for (int ch = 0; ch < NC; ++ch) {
                        for (int e = 0; e < 2; ++e) qd[e] += s_feat[r[e] * NCP + ch] * g[ch];
                    }
                    // a round's last pair may have no second member: row r0 + 1 is then stale (or never written: any bit
                    // pattern), and d = q - A with q = NaN would poison the chain — everything else of that half is masked
                    qd[1] = has1 ? qd[1] : 0.0f;
                }
                // ---- Gaussian 0 (the deeper one), then Gaussian 1: sequential in T and A (walk_entry) ----
                float dA[2], w[2], E[2];
                uint32_t gi[2];
                walk_entry<ST>(T, A, hit0, al[0], qd[0], dA[0], w[0]);
                walk_entry<ST>(T, A, hit1, al[1], qd[1], dA[1], w[1]);
                for (int e = 0; e < 2; ++e) E[e] = G[e] * dA[e];   // (0 for a miss)
                for (int e = 0; e < 2; ++e) gi[e] = s_cgid[r[e]];
                if constexpr (KV > 0) {
                    float red[2 * KV];   // [0, KV): entry 0, [KV, 2 KV): entry 1; of an entry: NV colours, the moments, the depth weight
#pragma unroll
                    for (int ch = 0; ch < NV; ++ch) {
                        for (int e = 0; e < 2; ++e) red[e * KV + ch] = w[e] * g[NM + ch];
                    }
                    // geometric partials as raw moments of E = G dL/dalpha over the pixel offset d;
                    // the per-Gaussian factors (conic, opacity, 0.5 W / 0.5 H) are applied once per
                    // Gaussian in preprocess_bwd instead of once per (pixel, Gaussian) here
                    if constexpr (!TM) {
                        for (int e = 0; e < 2; ++e) {
                            const float Ex = E[e] * dx[e], Ey = E[e] * dy[e];
                            red[e * KV + NV + 0] = Ex;
                            red[e * KV + NV + 1] = Ey;
                            red[e * KV + NV + 2] = Ex * dx[e];
                            red[e * KV + NV + 3] = Ex * dy[e];
                            red[e * KV + NV + 4] = Ey * dy[e];
                            red[e * KV + NV + 5] = E[e];
                        }
                    }
                    if constexpr (!XD && AUX) {
                        for (int e = 0; e < 2; ++e) red[e * KV + KV - 1] = w[e] * gD;
                    }
                    {
                        const float outv = wave_reduce_pack<2 * KV>(red, lane);
                        const uint32_t gid = slot_second ? gi[1] : gi[0];
                        if (slot_ok && (has1 || !slot_second)) rows.add(rows.index(gid, slot_stride, slot_off), outv);
                    }
                }
                if constexpr (MFMA) {
                    // park the weights (0 for pixels that miss); a pair never straddles a flush
                    for (int e = 0; e < 2; ++e) s_w[lane * WS + nslot + e] = w[e];
                    if constexpr (TM) {   // and E = G dL/dalpha in the 8-column panel (column = slot - e0)
                        for (int e = 0; e < 2; ++e) s_e[lane * ES + (nslot - e0) + e] = E[e];
                    }
                    if (lane == 0) {
                        for (int e = 0; e < 2; ++e) s_gid[nslot + e] = gi[e];
                        if constexpr (TM) {
                            for (int e = 0; e < 2; ++e) s_emean[nslot + e] = make_float2(p[e].x, p[e].y);
                        }
                    }
                    nslot += has1 ? 2 : 1;
                    if constexpr (TM) {
                        if (nslot - e0 >= EG - 1 || nslot >= GROUP - 1) {
                            reduce_e(nslot - e0);
                            e0 = nslot;
                        }
                    }
                    if (nslot >= GROUP - 1) {
                        flush_panel(nslot);
                        nslot = 0;
                        e0 = 0;
                    }
                }
            };
            // q[pix][g] = sum_ch F[g][ch] G[pix][ch] + z_g g_D for four staged rows on the matrix pipe:
            // v_mfma_f32_4x4x1_16b_f32 computes D[lane 4b+j][r] += A[lane 4b+r] * B[lane 4b+j]; with A =
            // feature of Gaussian (lane & 3) and B = this pixel's gradient, register r of every lane ends
            // up holding q[own pixel][Gaussian r].
            auto dot4 = [&](int slot4) -> f32x4 {
                const int k = lane & 3;
                const int srow = min(slot4 + k, ncand - 1);
                const float* fr = &s_feat[srow * NCP];
                const float zsel = reinterpret_cast<const float*>(&s_rec0[srow])[2];
                constexpr int CH = SR_BWD_DOT_CHAINS;   // independent accumulation chains
                f32x4 Qc[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) Qc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#if SR_BWD_DOT_PREFETCH
                // the next 16-byte piece of the row is requested before the four MFMAs of the current one
                const float4* f4 = reinterpret_cast<const float4*>(fr);
                float4 cur = f4[0];
#pragma unroll
                for (int i = 0; i < PPR; ++i) {
                    const float4 nxt = f4[i + 1 < PPR ? i + 1 : i];
                    const float v[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int ch = 4 * i + q;
                        if (ch < NC) Qc[ch % CH] = __builtin_amdgcn_mfma_f32_4x4x1f32(v[q], g[ch < NC ? ch : 0], Qc[ch % CH], 0, 0, 0);
                    }
                    cur = nxt;
                }
#else
#pragma unroll
                for (int ch = 0; ch < NC; ++ch)
                    Qc[ch % CH] = __builtin_amdgcn_mfma_f32_4x4x1f32(fr[ch], g[ch], Qc[ch % CH], 0, 0, 0);
#endif
                Qc[NC % CH] = __builtin_amdgcn_mfma_f32_4x4x1f32(zsel, gD, Qc[NC % CH], 0, 0, 0);
                f32x4 Q = Qc[0];
#pragma unroll
                for (int c = 1; c < CH; ++c) Q += Qc[c];
                return Q;
            };
#pragma unroll 1
            for (int slot = 0; slot < ncand; slot += (DOTM ? 4 : 2)) {
                // pop the next two (four) candidates, deepest first; hasK are wave-uniform
                const bool has1 = slot + 1 < ncand, has2 = DOTM && slot + 2 < ncand, has3 = DOTM && slot + 3 < ncand;
                const int j0 = 63 - __builtin_clzll(cand);
                cand &= ~(1ull << j0);
                const int j1 = has1 ? 63 - __builtin_clzll(cand) : j0;
                if (has1) cand &= ~(1ull << j1);
                const int j2 = has2 ? 63 - __builtin_clzll(cand) : j1;
                if (has2) cand &= ~(1ull << j2);
                const int j3 = has3 ? 63 - __builtin_clzll(cand) : j2;
                if (has3) cand &= ~(1ull << j3);
                float qm[4] = {0.f, 0.f, 0.f, 0.f};
                if (DOTM) {
                    const f32x4 Q = dot4(slot);
                    qm[0] = Q[0]; qm[1] = Q[1]; qm[2] = Q[2]; qm[3] = Q[3];
                }
                process_pair(j0, j1, has1, slot, slot + 1, qm[0], qm[1]);
                if (has2) process_pair(j2, j3, has3, slot + 2, slot + 3, qm[2], qm[3]);
            }
        }
    }
    if constexpr (TM) { if (nslot - e0 > 0) reduce_e(nslot - e0); }
    if (MFMA && nslot > 0) flush_panel(nslot);
}



static int g_small_panel_max_waves = SR_BWD_SMALL_PANEL_MAX_WAVES;
void set_small_panel_max_waves(int waves) { g_small_panel_max_waves = waves < 0 ? SR_BWD_SMALL_PANEL_MAX_WAVES : waves; }

struct BwdLaunch {
    const WinGrad* grads;
    const float* ckpt;   // non-null: split launch — SPLIT_PARTS waves per quadrant, wave k > 0 from the forward's segment records (common.h)
    int det_pass;        // deterministic mode: 0 = per-element max pass, 1 = fixed-point sum pass (acc_add)
};

template <int NC, bool DET, bool AUX = true>
static int launch_one_bwd(const FramePlan& p, int c0, int first, const BinView& b, const ImgView& im, const float* feat,
                          int feat_stride, const BwdLaunch& L, float* gacc, long long* gacc64, hipStream_t stream)
{
    const int gx = p.gx, tiles = p.tiles;
    const unsigned blocks = quadrant_blocks((int)p.gtiles, gx);  // 4 quadrants per (view, tile) (+ padding of the id space)
    const float* ckpt = (NC <= 4 && c0 == 0 && first) ? L.ckpt : nullptr;
    const GaccLayout GL = gacc_layout(p.C, p.P);
    if (NC == 35 && (c0 != 0 || GL.SH != 32u || GL.PV != 16u)) return SPLATRASTER_ERR_UNSUPPORTED;   // (the headline kernel's constants)
    // split launches with a launch order: three groups of extra workgroups (parts 4 .. 15 of the SPLIT_EXTRA_TILES longest lists) lead the grid
    const bool extras = ckpt != nullptr && p.order;
    const unsigned extra_blocks = extras ? (unsigned)(SPLIT_PARTS_MAX / SPLIT_PARTS - 1) * quadrant_blocks(SPLIT_EXTRA_TILES, gx) : 0u;
    const dim3 grid(blocks + extra_blocks, ckpt ? (unsigned)SPLIT_PARTS : 1u);
#define SR_BWD_LAUNCH(SPV)                                                                                          \
    hipLaunchKernelGGL((composite_bwd_kernel<NC, DET, SPV, AUX>), grid, dim3(WAVE), 0, stream, p.W,                     \
                       p.H, feat_stride, padded_channels(feat_stride) / 4, c0, first, tiles, p.V, p.P,                 \
                       b.ranges, b.ipack, b.irec, reinterpret_cast<const float4*>(feat), *L.grads,       \
                       im.final_T, im.n_contrib, gacc, GL,                                                             \
                       gacc_moment_offset(p.C), gacc64, ckpt, extras ? b.nparts : nullptr, (int)extra_blocks,                      \
                       p.order ? b.tile_order : nullptr, L.det_pass, p.dead_marks ? IPACK_REACH0 | IPACK_DEAD0 : IPACK_REACH0)
    if constexpr (NC >= 4 && NC <= 15 && AUX) {   // C = 3 and below: the flush costs what the 8 saved butterfly values gain (A/B: S0 0.036 vs 0.041 ms)
        // per VIEW: small frames (SplatLoc's 640x480) take the panel variant — also as a window of V views (A/B at the
        // reference layout, 5 views: 0.816 vs 0.869 ms); large frames the butterfly variant at full occupancy
        if (4 * tiles <= g_small_panel_max_waves)
            SR_BWD_LAUNCH(true);
        else
            SR_BWD_LAUNCH(false);
    } else {
        SR_BWD_LAUNCH(false);
    }
#undef SR_BWD_LAUNCH
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int launch_composite_bwd(const FramePlan& p, int64_t R, const BinView& b, const ImgView& im, const float* feat, int feat_stride,
                         const WinGrad& grads, float* gacc, long long* gacc64, int det_pass, hipStream_t stream)
{
    if (R == 0) return SPLATRASTER_OK;
    const bool det = gacc64 != nullptr;
    int C = p.C;
    const int V = p.V;
    // (the deterministic mode never splits; without the forward's segment records — p.split — nobody may)
    const BwdLaunch L{&grads, (!det && p.split) ? b.ckpt : nullptr, det_pass};
    // Channels and auxiliary planes that did not reach the loss are not computed: when the last channel's gradient
    // travels apart (grads.gc = C - 1) and NO view has one, the launch covers channels [0, C - 1) only — its dL/dfeature
    // column stays at the zero the accumulator rows were cleared to; without any depth / alpha gradient the RGB kernel
    // drops the depth weight from the dot product and the reduction (color_refinement: train_gaussians.py:283-285).
    bool any_last = false, any_aux = false;
    for (int v = 0; v < V; ++v) {
        any_last = any_last || grads.dL_dlast[v] != nullptr;
        any_aux = any_aux || grads.dL_ddepth[v] != nullptr || grads.dL_dalpha[v] != nullptr;
    }
    // (not in the deterministic mode: there the passes — and with them every rounding — do not depend on which outputs reached the
    //  loss; the kernel reads the last channel as the zeros a null dL_dlast stands for, and a launch is bit-identical to the one
    //  given the same gradient as full planes: tests/test_gpu_bwd_sources.py)
    if (grads.gc < C && !any_last && !det) C = grads.gc;
    if (C == 3 && !any_aux && !det)   // (the panel variant of this kernel measured equal at 640x480: 0.752 vs 0.760 ms per refinement iteration)
        return launch_one_bwd<3, false, false>(p, 0, 1, b, im, feat, feat_stride, L, gacc, gacc64, stream);
#define SR_BWD_ARGS b, im, feat, feat_stride, L, gacc, gacc64, stream
#define SR_BWD_ONE(N, c0_, first_) (det ? launch_one_bwd<N, true>(p, c0_, first_, SR_BWD_ARGS) : launch_one_bwd<N, false>(p, c0_, first_, SR_BWD_ARGS))
    if (C == 35) return SR_BWD_ONE(35, 0, 1);   // the headline layout has a kernel of its own; everything else is tiled greedily
    int c0 = 0, first = 1, st = SPLATRASTER_OK;
    while (c0 < C && st == SPLATRASTER_OK) {
        const int left = C - c0;
        if (left >= 32) { st = SR_BWD_ONE(32, c0, first); c0 += 32; }
        else if (left >= 16) { st = SR_BWD_ONE(16, c0, first); c0 += 16; }
        else if (left >= 8) { st = SR_BWD_ONE(8, c0, first); c0 += 8; }
        else if (left >= 4) { st = SR_BWD_ONE(4, c0, first); c0 += 4; }
        else if (left == 3) { st = SR_BWD_ONE(3, c0, first); c0 += 3; }
        else if (left == 2) { st = SR_BWD_ONE(2, c0, first); c0 += 2; }
        else { st = SR_BWD_ONE(1, c0, first); c0 += 1; }
        first = 0;
    }
#undef SR_BWD_ONE
#undef SR_BWD_ARGS
    return st;
}

}  // namespace sr

