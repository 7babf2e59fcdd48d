// mfma_tile.h — THE 32x32 tile of the exact-f32 MFMA v_mfma_f32_32x32x2_f32, for every kernel that multiplies matrices on it
// through the builtin (decoder.hip, retrieval.hip, netvlad_head.hip, conv2d.hip): the accumulator, its layout, the step of four k and
// the staging of two stacked operands, each written once.  composite_fwd.hip / composite_bwd.hip keep their in-place inline-asm
// forms.
//
// THE OPERAND CONTRACT of one D = A B + C with A [32][2], B [2][32], C and D [32][32], for lane (c = lane & 31, half = lane >> 5):
//   the lane's first operand is A[c][half], its second B[half][c]: one float each, so a kernel that walks k in pairs gives
//   half 0 the even k and half 1 the odd one;
//   register i of the lane's f32x16 holds D[acc_row(i, half)][c]: the column on the lane, the rows 4 half + 8 (i / 4) + i % 4;
//   D[r][c] = fmaf(A[r][1], B[1][c], fmaf(A[r][0], B[0][c], C[r][c])), one rounding per product and nothing wider inside.
// Accumulating through the same registers is therefore ONE fmaf chain per element, over k in the order the MFMAs are issued,
// starting from whatever the accumulator held (acc_zero: from zero).  Which kernel stages what, and how (LDS rows, float4s or
// scalars, VEC or not), never changes that chain: only the order of issue does.
#pragma once
#include "common.h"

namespace sr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row of accumulator register `reg`; the column is lane & 31
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ void acc_zero(f32x16& acc)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
}

// The k-quad step: four consecutive k of a lane's operand row as one float4 (x, y, z, w = k, k + 1, k + 2, k + 3).  pick() is the
// lane's share of it, .x for the first MFMA (k + half) and .y for the second (k + 2 + half); mfma_k4 issues the two, which
// advances the chain by four ascending k.  An operand shared by several accumulators is picked once, ahead of their loop.
// (By value: through a reference the quad is read again for every component, and decoder.hip's forward needs six registers more.)
__device__ __forceinline__ float2 pick(float4 q, int half) { return make_float2(half ? q.y : q.x, half ? q.w : q.z); }

__device__ __forceinline__ void mfma_k4(f32x16& acc, float2 a, float2 b)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
}

// The stacked two-operand tile: KC columns [k0, k0 + KC) of two row-major matrices that share the inner stride ld, rows
// [a0, a0 + RA) of `a` above rows [b0, b0 + RB) of `b`, as an LDS tile [ROWS][KC] at row stride LD (float4-aligned, off the bank
// period).  Staged element e = tid + THREADS i: row e / KC, column e % KC (VEC: float4 e, eight to a row); zero outside na, nb
// and ld.  fetch() loads into the struct's registers, stage() writes them to LDS a barrier later, so a chunk's loads fly under
// the MFMAs of the one before.  VEC needs ld % 4 == 0 and 16-byte aligned bases; both forms stage the same values.
// IDX is the width of the inner index: the caller's own, so its address arithmetic stays as wide as it was.
template <int THREADS, int RA, int RB, int KC, bool VEC>
struct StackedTile {
    static constexpr int ROWS = RA + RB, LD = KC + 4, PER_THREAD = ROWS * KC / THREADS;
    static_assert(KC == 32, "a row is 32 scalars or eight float4s");
    static_assert(ROWS * KC % THREADS == 0 && PER_THREAD % 4 == 0, "whole float4s per thread");
    float v[PER_THREAD];

    template <class IDX>
    __device__ __forceinline__ void fetch(const float* __restrict__ a, int64_t a0, int64_t na, const float* __restrict__ b, int64_t b0,
                                          int64_t nb, IDX ld, IDX k0, int tid)
    {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < PER_THREAD / 4; ++i) {
                const int e = tid + THREADS * i, row = e >> 3;
                const IDX kk = k0 + 4 * (e & 7);
                const bool isa = row < RA;
                const int64_t r = isa ? a0 + row : b0 + (row - RA);
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < (isa ? na : nb) && kk < ld) x = *reinterpret_cast<const float4*>((isa ? a : b) + r * ld + kk);
                v[4 * i] = x.x, v[4 * i + 1] = x.y, v[4 * i + 2] = x.z, v[4 * i + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < PER_THREAD; ++i) {
                const int e = tid + THREADS * i, row = e >> 5;
                const IDX kk = k0 + (e & 31);
                const bool isa = row < RA;
                const int64_t r = isa ? a0 + row : b0 + (row - RA);
                v[i] = (r < (isa ? na : nb) && kk < ld) ? (isa ? a : b)[r * ld + kk] : 0.f;
            }
        }
    }

    __device__ __forceinline__ void stage(float* lds, int tid) const
    {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < PER_THREAD / 4; ++i) {
                const int e = tid + THREADS * i;
                *reinterpret_cast<float4*>(lds + (e >> 3) * LD + 4 * (e & 7)) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PER_THREAD; ++i) {
                const int e = tid + THREADS * i;
                lds[(e >> 5) * LD + (e & 31)] = v[i];
            }
        }
    }
};

}  // namespace sr
