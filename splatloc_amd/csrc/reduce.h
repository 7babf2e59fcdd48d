// reduce.h — THE deterministic sums of the loss, densify and PnP stages: every sum of doubles (or ints) over a wave, over a
// block and over the block partials of an earlier launch goes through these, so its association order is written once:
//   wave:     the ascending xor butterfly, d = 1, 2, ... WAVE / 2 (every lane ends with the total);
//   block:    wave_sum per value, lane 0 of each wave stores s_red[wave][k], a barrier, then the wave partials are added in
//             ascending wave index; all in double;
//   partials: thread t adds partial[b][k] for b = t, t + THREADS, ... in that order, then the block (or wave) sum.
// wave_sum_f32 is the same butterfly over floats, for the NetVLAD head's norms (netvlad_head.hip); it has a name of its own so that
// no float argument of a wave_sum call, widened to double today, is ever captured by an overload.
// NOT for sums that associate differently — a float butterfly in another order rounds differently, and these results are
// compared bit for bit: pose.hip's L1 loss (descending float butterfly), decoder.hip's 32-lane butterfly32 and
// grid_encoding.hip's reductions keep their own code, as do the min / max reductions of knn.hip and fusion.hip, and image_ops.hip's
// sel_wave_sum (a descending __shfl_down sum of doubles: the frame statistics would round differently through the butterfly).
// The integer scans, ranks and selects, where no order matters, are scan.h.
#pragma once
#include "common.h"

namespace sr {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// first half of a block sum (the block has THREADS threads, all of them call): leaves the wave partials in s_red, behind a barrier
template <int THREADS, int K>
__device__ __forceinline__ void block_sum(const double (&acc)[K], double (&s_red)[THREADS / WAVE][K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE][k] = v;
    }
    __syncthreads();
}

// second half: value k of the block, for whichever thread(s) need it
template <int WAVES, int K>
__device__ __forceinline__ double block_total(const double (&s_red)[WAVES][K], int k)
{
    double t = 0;
    for (int w = 0; w < WAVES; ++w) t += s_red[w][k];
    return t;
}

// this thread's share of partial[blocks][K], the K sums of every block of an earlier launch
template <int THREADS, int K>
__device__ __forceinline__ void partials_sum(int blocks, const double* __restrict__ partial, double (&acc)[K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    for (int b = threadIdx.x; b < blocks; b += THREADS)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partial[(size_t)b * K + k];
}

// the K totals of partial[blocks][K], summed by one block of THREADS threads: total[] is valid in thread 0 only
template <int THREADS, int K>
__device__ __forceinline__ void partials_block_sum(int blocks, const double* __restrict__ partial,
                                                   double (&s_red)[THREADS / WAVE][K], double (&total)[K])
{
    double acc[K];
    partials_sum<THREADS>(blocks, partial, acc);
    block_sum<THREADS>(acc, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) total[k] = block_total(s_red, k);
}

}  // namespace sr
