// composite_common.h — pieces shared by the forward and backward compositing kernels: the reach test, the alpha arithmetic, the
// quadrant's frame, the split partition and the segment records (everything both passes must agree on), block ids, reductions.
#pragma once
#include <type_traits>

#include "common.h"

namespace sr {

// Conservative reach test of one projected Gaussian against the four 8x8 pixel quadrants of
// a 16x16 tile (bit q set <=> the Gaussian MAY reach alpha >= 1/255 at some pixel centre of
// quadrant q = (qx | qy << 1)).
//
// alpha = o * exp(power) >= 1/255  <=>  q(d) := A dx^2 + 2 B dx dy + C dy^2 <= 2 ln(255 o),
// and the minimum of the convex quadratic q over the quadrant's box of pixel centres is
// 0 if the centre lies inside, else attained on one of the four edges at the clamped 1-D
// minimiser.  The continuous box minimum is <= the minimum over pixel centres, and an
// absolute + relative slack far above fp32 / v_exp_f32 error is added, so a cleared bit
// proves that no pixel of the quadrant would pass the alpha >= 1/255 test: skipping the
// Gaussian for that wave leaves the image bit-identical.
__device__ __forceinline__ unsigned quadrant_reach_mask(const float4 r0, const float4 r1, float tile_x0,
                                                        float tile_y0)
{
    const float A = r1.x, B = r1.y, C = r1.z;
    const float lim0 = 2.0f * __logf(255.0f * r1.w);
    const float lim = lim0 + 0.02f + 1e-4f * fabsf(lim0);
    if (!(lim > 0.0f)) return 0u;
    const float nBrA = -B * __frcp_rn(A), nBrC = -B * __frcp_rn(C);
    unsigned mask = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float bx0 = tile_x0 + (float)((q & 1) * 8), by0 = tile_y0 + (float)((q >> 1) * 8);
        // d = mu - pixel: u in [u0, u1], v in [v0, v1]
        const float u0 = r0.x - (bx0 + 7.0f), u1 = r0.x - bx0;
        const float v0 = r0.y - (by0 + 7.0f), v1 = r0.y - by0;
        float qmin;
        if (u0 <= 0.0f && u1 >= 0.0f && v0 <= 0.0f && v1 >= 0.0f) {
            qmin = 0.0f;
        } else {
            qmin = 3.0e38f;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float ue = e ? u1 : u0;
                const float vs = fminf(v1, fmaxf(v0, nBrC * ue));
                qmin = fminf(qmin, A * ue * ue + 2.0f * B * ue * vs + C * vs * vs);
                const float ve = e ? v1 : v0;
                const float us = fminf(u1, fmaxf(u0, nBrA * ve));
                qmin = fminf(qmin, A * us * us + 2.0f * B * us * ve + C * ve * ve);
            }
        }
        if (qmin <= lim) mask |= 1u << q;
    }
    return mask;
}

// The per-instance payload stores the conic pre-scaled for the compositing kernels:
//   q = (-0.5 log2(e) A, -log2(e) B, -0.5 log2(e) C, opacity)
// so that log2 of the Gaussian weight is a 5-operation polynomial and the weight itself one
// v_exp_f32 (no separate -0.5 and log2(e) multiplies per (pixel, Gaussian)).  Forward and backward
// call the SAME function with explicit fmaf: their alpha values are bit-identical.
constexpr float LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float4 payload_conic(const float4& conic_opacity)
{
    return make_float4(-0.5f * LOG2E * conic_opacity.x, -LOG2E * conic_opacity.y, -0.5f * LOG2E * conic_opacity.z,
                       conic_opacity.w);
}
__device__ __forceinline__ float gauss_log2(const float4& q, float dx, float dy)
{
    return fmaf(dx, fmaf(q.y, dy, q.x * dx), (q.z * dy) * dy);
}
// 2^x as ONE explicit operation sequence that the CPU oracle restates instruction for instruction
// (its orc_exp2; the product never links it), so that alpha, the transmittance chain and therefore every
// alpha >= 1/255 / T < 1e-4 decision, n_contrib and final_T are BIT-IDENTICAL on both sides:
//   n = rint(x) (ties to even: v_rndne_f32), f = x - n in [-0.5, 0.5] (exact),
//   p = degree-5 minimax polynomial of 2^f (Horner, fmaf), result = ldexp(p, n) (v_ldexp_f32).
// c0 = 1 exactly (2^n is exact at the integers); max relative error 1.7e-7 (1.4 ulp) — the accuracy
// class of a libm expf.
// v_exp_f32 (the hardware approximation, 1 quarter-rate instruction instead of 9 full-rate ones) is
// not reproducible off the GPU; -DSR_EXP2_HW selects it for A/B timing only (cost: DESIGN.md §6.1).
constexpr float EXP2_C0 = 1.0f, EXP2_C1 = 0.6931470036506653f, EXP2_C2 = 0.24022242426872253f,
                EXP2_C3 = 0.05550733581185341f, EXP2_C4 = 0.009671512991189957f, EXP2_C5 = 0.001326472731307149f;
// The arithmetic without the argument clamp, for the compositing kernels (backward -2 % on S2 / S1 in round 3; the forward
// follows in round 4, two instructions per pair fewer, +0.3 % on S2): there the clamp's only job (an argument of -inf or
// NaN, reachable through an overflowing conic * d^2) is done for free by testing alpha BEFORE the min with 0.99 — NaN fails
// the >= 1/255 test, the Gaussian is a miss exactly as with the clamped 2^-200 = 0 — and by zeroing G, not dL/dalpha, for a
// miss in the backward.  For every finite argument the value is the clamped function's, bit for bit: below -200 both flush to
// 0 in v_ldexp_f32, above 0 the pixel is skipped (power > 0) whatever comes out.  v_cvt_i32_f32 saturates and maps NaN to 0;
// it is written as asm because an out-of-range float -> int conversion is undefined in C++.
__device__ __forceinline__ float exp2_core(float x)
{
#ifdef SR_EXP2_HW
    return __builtin_amdgcn_exp2f(x);
#else
    const float n = __builtin_rintf(x);
    const float f = x - n;
    float p = fmaf(EXP2_C5, f, EXP2_C4);
    p = fmaf(p, f, EXP2_C3);
    p = fmaf(p, f, EXP2_C2);
    p = fmaf(p, f, EXP2_C1);
    p = fmaf(p, f, EXP2_C0);
    int e;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(e) : "v"(n));
    return __builtin_amdgcn_ldexpf(p, e);
#endif
}
__device__ __forceinline__ float exp2_shared(float x)
{
    // clamp first, exactly like orc_exp2: x = -inf would make f = NaN (and min(0.99, o * NaN) = 0.99, a spurious
    // opaque hit), and (int)n of an out-of-range float is undefined.  2^-200 flushes to 0 in ldexp either way.
    return exp2_core(fminf(fmaxf(x, -200.0f), 200.0f));
}
// T (1 - alpha) with two roundings, never a contracted fma: the oracle's transmittance chain
__device__ __forceinline__ float transmit(float T, float alpha)
{
#pragma clang fp contract(off)
    const float om = 1.0f - alpha;
    return T * om;
}

// Block id -> (global tile, quadrant) for the wave-per-quadrant kernels.  Observed dispatch: block b -> XCD b % 8, in
// order of b within an XCD.  The four quadrants of a tile get ids with the same (id % 8): they run on the same
// XCD and share its L2 for the tile's list; consecutive tiles are interleaved over the XCDs, which balances the
// load and spreads the atomics of one Gaussian over time (mapping every XCD to its own contiguous band of tiles
// was measured slower: forward 0.476 vs 0.419 ms, backward 0.982 vs 0.853 ms on S2).  Speed only, never correctness.
// `order` (binning.hip tile_order_kernel; null = identity) turns the tile slot into the tile that runs there: longest lists first.
__device__ __forceinline__ void quadrant_of_block(unsigned id, int tiles, int gx, int& tile, int& quad,
                                                  const uint32_t* __restrict__ order = nullptr)
{
    (void)gx;
    tile = (int)((id >> 5) * 8u + (id & 7u));
    quad = (int)((id >> 3) & 3u);
    if (order && tile < tiles) tile = (int)order[tile];
}
// blocks to launch so that every tile's four quadrants get an id
__host__ __device__ static inline unsigned quadrant_blocks(int tiles, int gx)
{
    (void)gx;
    return (unsigned)((tiles + 7) / 8) * 32u;
}

// ---- what the forward and the backward must agree on: each is written once, here ---------------------------------
// The forward's three walkers (composite_fwd.hip) and the backward (composite_bwd.hip) build their quadrant's frame, evaluate alpha
// and its two tests, cut a split list into parts and address a segment record through these bodies and no others.

__device__ __forceinline__ int tile_columns(int W) { return (W + TILE - 1) / TILE; }

// what a wave knows about its 8x8 quadrant of global tile `gtile` (= view * tiles + tile) and about its lane's pixel in it
struct QuadFrame {
    int view;            // wave-uniform (scalar)
    uint32_t row0;       // the view's first row: feature row of row g is g - row0
    int qx, qy, px, py;  // the quadrant's and the lane's first / own pixel
    bool inside;
    uint32_t beg, end;   // the tile's list
    size_t plane, pix;   // H * W; the pixel's offset in a plane
};
__device__ __forceinline__ QuadFrame quadrant_frame(int W, int H, int tiles, int V, int P, const uint32_t* __restrict__ ranges, int gtile,
                                                    int quad, int lane)
{
    QuadFrame F;
    const int gx = tile_columns(W);
    F.view = (V == 1) ? 0 : gtile / tiles;
    const int tile = gtile - F.view * tiles;
    F.row0 = (uint32_t)F.view * (uint32_t)P;
    F.qx = (tile % gx) * TILE + (quad & 1) * 8, F.qy = (tile / gx) * TILE + (quad >> 1) * 8;
    F.px = F.qx + (lane & 7), F.py = F.qy + (lane >> 3);
    F.inside = F.px < W && F.py < H;
    F.beg = ranges[2 * gtile], F.end = ranges[2 * gtile + 1];
    F.plane = (size_t)H * W;
    F.pix = (size_t)F.py * W + F.px;
    return F;
}

// the packed word (id | reach bits << 24) of list entry `at`; 0 (reaches nothing) behind the list's end
__device__ __forceinline__ uint32_t list_word(const uint32_t* __restrict__ ipack, uint32_t at, uint32_t end) { return at < end ? ipack[at] : 0u; }

// alpha of two Gaussians (q: pre-scaled conic, opacity) at offsets d = centre - pixel, and whether each passes the tests.  Alpha is
// tested BEFORE the min with 0.99: a NaN from an overflowed power is a miss, which is the only thing the argument clamp of exp2_shared
// was there for.  The absent candidate (opacity 0) never passes.  G = the raw weight 2^power, which the backward multiplies dL/dalpha
// with (zeroed there for a miss: G, not dL/dalpha — the same NaN); the forward leaves it unused.
struct PairAlpha { float al0, al1; bool pass0, pass1; float G0, G1; };
__device__ __forceinline__ PairAlpha pair_alpha(const float4& q0, float dx0, float dy0, const float4& q1, float dx1, float dy1)
{
    const float pw0 = gauss_log2(q0, dx0, dy0), pw1 = gauss_log2(q1, dx1, dy1);  // log2 of the weight
    const float G0 = exp2_core(pw0), ar0 = q0.w * G0, G1 = exp2_core(pw1), ar1 = q1.w * G1;
    return {fminf(ALPHA_MAX, ar0), fminf(ALPHA_MAX, ar1), pw0 <= 0.0f && ar0 >= ALPHA_MIN, pw1 <= 0.0f && ar1 >= ALPHA_MIN, G0, G1};
}

// ---- split launches (common.h): the backward runs several waves per quadrant, one per part of the list.  Segment record k
// = { T in front of the segment's first entry, the colours and the depth the segment ALONE contributes } — segment sums are
// accumulated from zero, so they are accurate relative to their own (transmittance-scaled) magnitude; the backward rebuilds "what
// lies behind a boundary" from the sums of the later segments (a prefix C_k subtracted from the image would carry the image's
// rounding, 1e-7 |C|, into a remainder of size T_k |C|).
// THE partition of a split list of `len` entries: part k = entries [k part, (k + 1) part) of the list, the last part to its end
struct SplitParts {
    int np;         // parts of this list (wave-uniform)
    uint32_t part;  // entries per part; 0: not a split launch
};
__device__ __forceinline__ SplitParts split_parts(bool split, const uint32_t* __restrict__ nparts, int gtile, uint32_t len)
{
    SplitParts s;
    s.np = (split && nparts != nullptr) ? (int)nparts[gtile] : SPLIT_PARTS;
    s.part = split ? split_part(len, (uint32_t)s.np) : 0u;
    return s;
}
// the backward's wave of part k: [beg, end) shrinks from the list to that part
__device__ __forceinline__ void take_part(const SplitParts& s, int k, uint32_t& beg, uint32_t& end)
{
    beg += (uint32_t)k * s.part;
    if (k < s.np - 1) end = min(end, beg + s.part);
}
// the forward walks all parts in one go
struct SplitCursor {
    int np;         // parts of this list (wave-uniform)
    uint32_t part;  // entries per part; 0: not a split launch
    uint32_t at;    // the entry the current segment ends in front of
    int k;          // the current segment
};
__device__ __forceinline__ SplitCursor split_cursor(const float* ckpt_all, const uint32_t* __restrict__ nparts, int gtile, uint32_t beg,
                                                    uint32_t end)
{
    const SplitParts s = split_parts(ckpt_all != nullptr, nparts, gtile, end - beg);
    SplitCursor c;
    c.np = s.np;
    c.part = s.part;
    c.at = c.part ? beg + c.part : 0xFFFFFFFFu;
    c.k = 0;
    return c;
}
// a segment ends in front of entry `base`: the cursor moves on to the next one (the segment that ended is c.k - 1)
__device__ __forceinline__ bool segment_ends(SplitCursor& c, uint32_t base)
{
    if (base != c.at) return false;
    ++c.k;
    c.at = c.k < c.np - 1 ? c.at + c.part : 0xFFFFFFFFu;
    return true;
}
// plane `pl` of the pixel's segment record k: ckpt_all is [V][SPLIT_PARTS_MAX][nc + 2][H * W], plane 0 = T, 1 .. nc colours, nc + 1 depth.
// nc = the channels of the LAUNCH: the forward's template constant, handed over as Channels<NC> (a type, so that the record's stride is
// a constant where the address is formed); the backward's runtime C_total, whose pass may cover fewer.  F32 = float for the forward,
// which writes the records, const float for the backward.
template <int N>
using Channels = std::integral_constant<int, N>;
template <typename F32, typename Count>
__device__ __forceinline__ F32* segment_record(F32* __restrict__ ckpt_all, const QuadFrame& F, Count nc, int k, int pl)
{
    return ckpt_all + (((size_t)F.view * SPLIT_PARTS_MAX + k) * (nc + 2) + pl) * F.plane + F.pix;
}

// ---- DPP helpers (wave64 = 4 rows of 16 lanes) -----------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_get(float v)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

// ---- packed butterfly reduction -----------------------------------------------------------
// Reduces K per-lane values over the 64 lanes of a wave and leaves total k in lane
// bitreverse6(k): every stage halves the lane span of each value AND merges two registers
// into one, so the whole reduction costs ~2.2 VALU per value instead of 6 DPP adds + a
// readlane/select gather per value.
//   stage 1 (lane bit 5): v_permlane32_swap + add      (2 instr per pair)
//   stage 2 (lane bit 4): v_permlane16_swap + add      (2 instr per pair)
//   stage 3 (lane bit 3): two bank-masked v_add_f32_dpp row_ror:8       (fold_lane_bit3)
//   stage 4 (lane bit 2): two bank-masked v_add_f32_dpp row_ror:12 / 4   (fold_lane_bit2)
//   stage 5 (lane bit 1): select / select / add quad_perm[2,3,0,1]
//   stage 6 (lane bit 0): select / select / add quad_perm[1,0,3,2]
__device__ __forceinline__ float as_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_u(float f) { return __builtin_bit_cast(unsigned, f); }

template <int CTRL, int BANK_MASK>
__device__ __forceinline__ float dpp_mov_old(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                 __builtin_bit_cast(int, v), CTRL, 0xf,
                                                                 BANK_MASK, false));
}

// One stage of the packed butterfly on lane bit 3 / bit 2: lanes with the bit clear end with x + x[partner], lanes with it
// set with y + y[partner] (partner = lane ^ 8 / lane ^ 4).  Both bits are constant inside a DPP bank (4 lanes), so each half is
// ONE bank-masked v_add_f32_dpp on the untouched inputs — 2 instructions per output instead of select / select / (moves) / add
// (3 for bit 3, 6 for bit 2).  s_nop 1 = the two wait states a DPP read of a just-written VGPR needs (the compiler cannot see
// into the asm).
#ifndef SR_BUTTERFLY_ASM
#define SR_BUTTERFLY_ASM 1   // 0 = the select / move formulation through compiler builtins (A/B)
#endif
__device__ __forceinline__ float fold_lane_bit3(float x, float y)
{
#if !SR_BUTTERFLY_ASM
    const bool lo = (__lane_id() & 8) == 0;
    const float keep = lo ? x : y, send = lo ? y : x;
    return keep + dpp_get<0x128, 0xf>(send);
#endif
    float d;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc"
        : "=&v"(d)
        : "v"(x), "v"(y));
    return d;
}
__device__ __forceinline__ float fold_lane_bit2(float x, float y)
{
#if !SR_BUTTERFLY_ASM
    const bool lo = (__lane_id() & 4) == 0;
    const float keep = lo ? x : y, send = lo ? y : x;
    float t = dpp_mov_old<0x12C, 0x5>(0.0f, send);
    t = dpp_mov_old<0x124, 0xA>(t, send);
    return keep + t;
#endif
    float d;   // banks 0, 2 (bit clear) read lane + 4 = row_ror:12; banks 1, 3 read lane - 4 = row_ror:4
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xa"
        : "=&v"(d)
        : "v"(x), "v"(y));
    return d;
}

template <int K>
__device__ __forceinline__ float wave_reduce_pack(const float (&v)[K], int lane)
{
    static_assert(K >= 1 && K <= 64, "at most 64 values per wave");
    constexpr int N1 = (K + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2,
                  N5 = (N4 + 1) / 2, N6 = (N5 + 1) / 2;
    static_assert(N6 == 1, "");
    float a[N1];
#pragma unroll
    for (int m = 0; m < N1; ++m) {
        const float x = v[2 * m];
        const float y = (2 * m + 1 < K) ? v[2 * m + 1] : 0.0f;
        const auto r = __builtin_amdgcn_permlane32_swap(as_u(x), as_u(y), false, false);
        a[m] = as_f(r[0]) + as_f(r[1]);
    }
    float b[N2];
#pragma unroll
    for (int m = 0; m < N2; ++m) {
        const float x = a[2 * m];
        const float y = (2 * m + 1 < N1) ? a[2 * m + 1] : 0.0f;
        const auto r = __builtin_amdgcn_permlane16_swap(as_u(x), as_u(y), false, false);
        b[m] = as_f(r[0]) + as_f(r[1]);
    }
    float c[N3];
#pragma unroll
    // A stage's last register may have no partner value (odd count): the lanes that would hold it then belong to value
    // indices >= K, which no caller consumes (and which never feed a lane of an existing index: later stages pair lanes
    // that agree in all higher bits) — there x + x[partner] in every lane is one instruction.
    for (int m = 0; m < N3; ++m)
        c[m] = (2 * m + 1 < N2) ? fold_lane_bit3(b[2 * m], b[2 * m + 1 < N2 ? 2 * m + 1 : 0]) : b[2 * m] + dpp_get<0x128, 0xf>(b[2 * m]);
    float d[N4];
#pragma unroll
    for (int m = 0; m < N4; ++m)
        d[m] = (2 * m + 1 < N3) ? fold_lane_bit2(c[2 * m], c[2 * m + 1 < N3 ? 2 * m + 1 : 0]) : fold_lane_bit2(c[2 * m], c[2 * m]);
    float e[N5];
    {
        const bool lo = (lane & 2) == 0;
#pragma unroll
        for (int m = 0; m < N5; ++m) {
            const float x = d[2 * m];
            if (2 * m + 1 < N4) {
                const float y = d[2 * m + 1 < N4 ? 2 * m + 1 : 0];
                const float keep = lo ? x : y, send = lo ? y : x;
                e[m] = keep + dpp_get<0x4E, 0xf>(send);  // quad_perm [2,3,0,1]
            } else {
                e[m] = x + dpp_get<0x4E, 0xf>(x);
            }
        }
    }
    const float x6 = e[0];
    if (N5 > 1) {
        const bool lo1 = (lane & 1) == 0;
        const float y6 = e[N5 > 1 ? 1 : 0];
        const float keep6 = lo1 ? x6 : y6, send6 = lo1 ? y6 : x6;
        return keep6 + dpp_get<0xB1, 0xf>(send6);  // quad_perm [1,0,3,2]
    }
    return x6 + dpp_get<0xB1, 0xf>(x6);
}

// The first three stages of wave_reduce_pack only: K <= 8 per-lane values are summed over lane bits 5, 4, 3 (lanes that
// differ in bits 0..2 stay separate); lane l ends with the total of value (l >> 5 & 1) + 2 (l >> 4 & 1) + 4 (l >> 3 & 1).
template <int K>
__device__ __forceinline__ float wave_reduce_hi3(const float (&v)[K], int lane)
{
    static_assert(K >= 1 && K <= 8, "at most 8 values");
    constexpr int N1 = (K + 1) / 2, N2 = (N1 + 1) / 2;
    float a[N1];
#pragma unroll
    for (int m = 0; m < N1; ++m) {
        const float x = v[2 * m];
        const float y = (2 * m + 1 < K) ? v[2 * m + 1] : 0.0f;
        const auto r = __builtin_amdgcn_permlane32_swap(as_u(x), as_u(y), false, false);
        a[m] = as_f(r[0]) + as_f(r[1]);
    }
    float b[N2];
#pragma unroll
    for (int m = 0; m < N2; ++m) {
        const float x = a[2 * m];
        const float y = (2 * m + 1 < N1) ? a[2 * m + 1] : 0.0f;
        const auto r = __builtin_amdgcn_permlane16_swap(as_u(x), as_u(y), false, false);
        b[m] = as_f(r[0]) + as_f(r[1]);
    }
    (void)lane;
    if (N2 > 1) return fold_lane_bit3(b[0], b[N2 > 1 ? 1 : 0]);
    return b[0] + dpp_get<0x128, 0xf>(b[0]);
}

}  // namespace sr
