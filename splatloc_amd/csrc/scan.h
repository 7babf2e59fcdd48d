// scan.h — THE integer scans, ranks and selects of the sort, binning, frame-preparation, SuperPoint and retrieval stages, each
// written once (reduce.h does the same for the deterministic floating-point sums):
//   lanes_below:          the ballot mask of the lanes in front of this one (ranks among equal digits, in-place compaction);
//   wave_inclusive_scan:  the __shfl_up ladder, d = 1, 2, ... WAVE / 2, for uint32_t and uint64_t;
//   block_exclusive_scan: the wave scan, the last lane of each wave stores s_wsum[wave], ONE barrier, then every thread adds the
//                         sums of the waves in front of its own (and, on request, all of them: the workgroup's total);
//   float_order_key:      a float as the uint32_t that orders like it, and back;
//   radix_pick:           one wave finds the digit whose bin holds rank k (0-based) of 256 counts, walked up or down;
//   radix_select_block:   the four-pass radix select of one workgroup over 32-bit keys, built from an LDS histogram and that pick.
// All of it is integer arithmetic: no result depends on the order in which these add.
// NOT through here: retrieval.hip's wave_insert (a shift by one lane, not a scan), the min / max ladders of knn.hip and fusion.hip,
// the ballot prefixes of composite_fwd.hip and matching.hip (their own masks, left with their kernels), sel_wave_sum of
// image_ops.hip (a sum of doubles: reduce.h says why it stays), and the two scans per step of sp_pick_kernel's walk
// (superpoint_head.hip's sp_walk_scan: at sixteen waves block_exclusive_scan adds the wave sums in a loop of dependent LDS
// reads, and with two scans in each of the walk's steps the kernel measured 28.4 us for 21.0; wave 0 scanning the wave sums,
// at two barriers more, is the faster form there).  The digit-rank body of the LSD sort lives in scan_sort.hip, its
// only user.
#pragma once
#include "common.h"

namespace sr {

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (lane == 0) ? 0ull : (~0ull >> (WAVE - lane)); }

// every lane of the wave calls; lane l returns v(0) + ... + v(l)
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "uint32_t or uint64_t");
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T t = __shfl_up(v, d, WAVE);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of THREADS threads (all of them call); s_wsum: THREADS / WAVE values of
// LDS.  `total`, when given, receives the sum over the workgroup in every thread — a caller that scans in steps adds it to its
// running carry.
// Barriers: exactly one, between the store of the wave sums and their reads.  s_wsum is NOT free on return (slower waves are still
// reading it): a caller that writes it again — a second call, the next step of a loop — takes a barrier of its own first.
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s_wsum, T* total = nullptr)
{
    constexpr int NW = THREADS / WAVE;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const T incl = wave_inclusive_scan(v);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_wsum[w] = incl;
    __syncthreads();
    T before = 0, all = 0;
    // four waves: no loop.  Sixteen: two wave sums in flight — measured, not a guess: fully unrolled sp_pick_kernel needs 64 VGPRs
    // for 22 and sp_offsets_kernel 45 for 18, four at a time sp_offsets_kernel still 20; two keeps every caller at or below its own
    // former code (HISTORY.md §29)
    constexpr int UNROLL = NW <= 4 ? NW : 2;
#pragma unroll UNROLL
    for (int k = 0; k < NW; ++k) {
        const T c = s_wsum[k];
        before += (k < w) ? c : (T)0;
        all += c;
    }
    if (total) *total = all;
    return before + incl - v;
}

// larger float <=> larger key (-0 below +0; NaNs at the two ends, by their sign)
__device__ __forceinline__ uint32_t float_order_key(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_from_order_key(uint32_t key)
{
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// All 64 lanes of one wave: the digit whose bin holds rank k (0-based) of the 256 counts walked from digit 0 up (from digit 255
// down when DESCENDING), the rank left inside that bin, and the total.  `median`: k = (total - 1) / 2, whatever was passed.
// With k beyond the total (an empty histogram) the digit and the rank are 0.
template <bool DESCENDING>
__device__ __forceinline__ void radix_pick(const uint32_t* hist, bool median, uint32_t k, uint32_t* digit, uint32_t* rank, uint32_t* total)
{
    const int lane = threadIdx.x & (WAVE - 1);
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = hist[DESCENDING ? 255 - (4 * lane + j) : 4 * lane + j];
    const uint32_t s = (c[0] + c[1]) + (c[2] + c[3]);
    const uint32_t incl = wave_inclusive_scan(s);
    const uint32_t tot = __shfl(incl, WAVE - 1);
    if (median) k = tot ? (tot - 1) / 2 : 0;
    const uint32_t excl = incl - s;
    const bool mine = excl <= k && k < incl;
    uint32_t dg = 0, kr = 0;
    if (mine) {
        uint32_t cum = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k < cum + c[j]) {
                dg = DESCENDING ? 255 - (4 * lane + j) : 4 * lane + j;
                kr = k - cum;
                break;
            }
            cum += c[j];
        }
    }
    const unsigned long long owners = __ballot(mine);
    const int src = owners ? __ffsll((long long)owners) - 1 : 0;
    *digit = __shfl(dg, src);
    *rank = __shfl(kr, src);
    *total = tot;
}

// One workgroup of THREADS >= 256 threads (all of them call): the key of rank k (0-based; ascending, or descending) among
// key_at(0) ... key_at(n - 1), most significant byte first.  Returns the key; *rank_left (when given): its rank among the keys equal to it.
// s_hist: 256 words, s_sel: 2 words of LDS.  key_at is called once per key and pass.
// Barriers: three per pass, the last one behind the pick — s_hist and s_sel are free on return, and whatever the caller wrote to
// LDS before the call is complete behind the first.  `first_barrier`, when given, IS the barrier behind the first pass's histogram
// (every thread has seen each of its keys once by then): a caller with a vote to take over the keys passes a functor that takes
// it as that barrier (__syncthreads_or ...), instead of paying for a barrier of its own.
struct plain_barrier {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
template <int THREADS, bool DESCENDING, typename KeyAt, typename FirstBarrier = plain_barrier>
__device__ __forceinline__ uint32_t radix_select_block(uint32_t n, KeyAt key_at, uint32_t k, uint32_t* s_hist, uint32_t* s_sel,
                                                       uint32_t* rank_left = nullptr, FirstBarrier first_barrier = FirstBarrier())
{
    static_assert(THREADS >= 256, "one thread per bin");
    const uint32_t tid = threadIdx.x;
    uint32_t prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const uint32_t hi = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (uint32_t i = tid; i < n; i += THREADS) {
            const uint32_t u = key_at(i);
            if ((u & hi) == prefix) atomicAdd(&s_hist[(u >> shift) & 255u], 1u);
        }
        if (shift == 24)
            first_barrier();
        else
            __syncthreads();
        if (tid < WAVE) {
            uint32_t digit, rank, total;
            radix_pick<DESCENDING>(s_hist, false, k, &digit, &rank, &total);
            if (tid == 0) {
                s_sel[0] = prefix | (digit << shift);
                s_sel[1] = rank;
            }
        }
        __syncthreads();
        prefix = s_sel[0];
        k = s_sel[1];
    }
    if (rank_left) *rank_left = k;
    return prefix;
}

}  // namespace sr
