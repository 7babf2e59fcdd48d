// scan_sort.hip — device-wide prefix sum and stable LSD radix sort, hand-written for
// wave64 (no rocPRIM / hipCUB).  Replaces cub::DeviceScan::InclusiveSum and
// cub::DeviceRadixSort::SortPairs of the rasterizer lineage.
//
// Sort: 8-bit digits, 256-thread blocks (4 wave64), 4096 keys per block.
//   pass = histogram kernel  -> [digit][block] table
//          exclusive scan of the table (the scan below)
//          scatter kernel: wave-level multi-way match (8 ballots) gives each key its
//          stable rank among equal digits; per-wave digit counters live in LDS.
// Stability: keys are consumed in (block, wave, iteration, lane) order == memory order.
// Both kernels are HBM-bound: per pass 2 key reads + 1 value read + 1 key/value write.
#include <mutex>

#include "common.h"
#include "scan.h"

namespace sr {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

constexpr int SORT_THREADS = 256;
#ifndef SR_SORT_LOOKBACK
#define SR_SORT_LOOKBACK 8  // predecessors whose status words are loaded together in the look-back
#endif
#ifndef SR_SORT_ITEMS
#define SR_SORT_ITEMS 16
#endif
constexpr int SORT_ITEMS = SR_SORT_ITEMS;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;  // 4096
constexpr int SORT_WAVES = SORT_THREADS / WAVE;
constexpr int RADIX = 256;

// ---------------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------------
// in[perm[i]] without the random gather: the permutation's words carry min(in[row], 255) in bits 24..31 (rows are
// < 2^24: capi.hip), so only the rare large values (a Gaussian over >= 255 tiles) are looked up.  The plain gather of
// 4-byte words over 2.5 M rows cost 64 us per window (64-byte sectors: 160 MB of traffic for 10 MB of data).
__device__ __forceinline__ uint32_t perm_value(const uint32_t* __restrict__ in, uint32_t p)
{
    const uint32_t t = p >> 24;
    return t < 255u ? t : in[p & 0xFFFFFFu];
}
__global__ void __launch_bounds__(SCAN_THREADS)
scan_reduce_kernel(int64_t n, const uint32_t* __restrict__ in, const uint32_t* __restrict__ perm,
                   uint64_t* __restrict__ partial)
{
    __shared__ uint64_t wsum[SCAN_THREADS / WAVE];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int64_t i = base + (int64_t)k * SCAN_THREADS + threadIdx.x;
        if (i < n) s += perm ? perm_value(in, perm[i]) : in[i];
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) s += __shfl_down(s, d, WAVE);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) wsum[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int k = 0; k < SCAN_THREADS / WAVE; ++k) t += wsum[k];
        partial[blockIdx.x] = t;
    }
}

// one block: exclusive scan of partial[0..nb) in place; total written as u64
__global__ void __launch_bounds__(1024)
scan_partials_kernel(int64_t nb, uint64_t* __restrict__ partial, uint64_t* __restrict__ total)
{
    __shared__ uint64_t wsum[1024 / WAVE];
    uint64_t carry = 0;
    for (int64_t start = 0; start < nb; start += 1024) {
        const int64_t i = start + threadIdx.x;
        const uint64_t v = i < nb ? partial[i] : 0;
        uint64_t step;
        const uint64_t excl = block_exclusive_scan<1024>(v, wsum, &step);
        if (i < nb) partial[i] = carry + excl;
        carry += step;
        __syncthreads();   // (the next step overwrites the wave sums)
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

template <bool EXCLUSIVE>
__global__ void __launch_bounds__(SCAN_THREADS)
scan_apply_kernel(int64_t n, const uint32_t* in, const uint32_t* __restrict__ perm,
                  const uint64_t* __restrict__ partial, uint32_t* out)  // in may alias out
{
    __shared__ uint32_t wsum[SCAN_THREADS / WAVE];
    // blocked arrangement: thread t owns items [t*ITEMS, (t+1)*ITEMS)
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int64_t i = base + k;
        v[k] = i < n ? (perm ? perm_value(in, perm[i]) : in[i]) : 0u;
        s += v[k];
    }
    uint32_t run = (uint32_t)partial[blockIdx.x] + block_exclusive_scan<SCAN_THREADS>(s, wsum);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int64_t i = base + k;
        if (EXCLUSIVE) {
            if (i < n) out[i] = run;
            run += v[k];
        } else {
            run += v[k];
            if (i < n) out[i] = run;
        }
    }
}

// ---- look-back watchdog ------------------------------------------------------------------
// The decoupled look-backs below spin on predecessors that already hold a ticket, so they always
// make progress on a healthy GPU.  They never give up with a partial prefix — a wrong prefix would be
// a silently mis-sorted frame, and garbage offsets send the downstream kernels out of bounds.  Two bounds:
//   soft (g_spin_limit, default 2^24 spins): the block raises a flag in HOST-mapped pinned memory
//        (system-scope store) and KEEPS WAITING.  Results are late, never wrong, so this is NOT an error of
//        any frame: only splatraster_poll_errors() reports it (SPLATRASTER_WARN_LOOKBACK_STALL) — forward /
//        backward keep returning OK for their correct results;
//   hard (2^30 spins, minutes): the predecessor is never going to publish (wedged device / lost block).
//        The block executes s_trap: the kernel aborts and every later HIP call on the device returns an
//        error, which the C ABI surfaces as SPLATRASTER_ERR_HIP — a wedge is a fault, not a silent hang.
// The soft bound is a device global so that tests/test_gpu_edge_cases.py can force the report
// (splatraster_debug_set_spin_limit).
constexpr uint32_t SPIN_HARD_LIMIT = 1u << 30;
__device__ uint32_t* g_err_sink = nullptr;          // device address of the host flag word
__device__ uint32_t g_spin_limit = 1u << 24;

__device__ __forceinline__ void lookback_timeout(uint32_t* state_error)
{
    *state_error = 1u;
    uint32_t* sink = g_err_sink;
    if (sink) __hip_atomic_store(sink, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int MAX_DEVICES = 64;
static uint32_t* g_err_host[MAX_DEVICES] = {};       // pinned, mapped; one word per device
static std::mutex g_err_mu;                          // several host threads may make their first call at once

int lookback_error_init()
{
    int dev = 0;
    SR_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return SPLATRASTER_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_err_mu);
    if (g_err_host[dev]) return SPLATRASTER_OK;
    uint32_t* h = nullptr;
    SR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h), 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent));
    *h = 0u;
    uint32_t* d = nullptr;
    SR_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0));
    SR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_err_sink), &d, sizeof(d)));
    g_err_host[dev] = h;
    return SPLATRASTER_OK;
}

// SPLATRASTER_WARN_LOOKBACK_STALL once for every raised soft flag (the flag is cleared), else OK.  Only
// splatraster_poll_errors() calls this: a soft stall never fails the frame that was late.
int lookback_error_poll()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return SPLATRASTER_OK;
    volatile uint32_t* h;
    {
        std::lock_guard<std::mutex> lk(g_err_mu);
        h = g_err_host[dev];
    }
    if (!h || *h == 0u) return SPLATRASTER_OK;
    *h = 0u;
    set_error_text("look-back watchdog: a scan / radix-sort block waited longer than the spin bound for a predecessor (stalling device); results are late, never wrong");
    return SPLATRASTER_WARN_LOOKBACK_STALL;
}

int lookback_set_spin_limit(uint32_t limit)
{
    SR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_spin_limit), &limit, sizeof(limit)));
    return SPLATRASTER_OK;
}

// One-pass inclusive scan (n <= SCAN_ONEPASS_MAX_BLOCKS tiles): each block scans its tile, publishes
// its total in a 64-bit status word (value | flag << 62: 1 = tile total, 2 = inclusive prefix) and
// wave 0 resolves the exclusive prefix with a wave-wide decoupled look-back — 64 predecessors per
// L2 round trip.  Relaxed agent-scope atomics (the word IS the flag), ticketed block ids (a block
// only waits for blocks that already started), bounded spins.  State (ticket + status words) must
// be zero on entry.
constexpr int SCAN_ONEPASS_MAX_BLOCKS = 2048;
constexpr uint64_t SC_LOCAL = 1ull << 62, SC_INCL = 2ull << 62, SC_VAL = (1ull << 62) - 1ull;

struct ScanState {
    uint32_t ticket;
    uint32_t error;
    uint64_t status[1];  // [nb]
};

template <bool EXCLUSIVE>
__global__ void __launch_bounds__(SCAN_THREADS)
scan_onepass_kernel(int64_t n, const uint32_t* in, const uint32_t* __restrict__ perm,
                    uint32_t* out /* may alias in */, uint64_t* __restrict__ total, ScanState* __restrict__ st,
                    uint32_t* __restrict__ span_owner /* or NULL */, uint32_t span, uint32_t span_cap)
{
    __shared__ uint32_t wsum[SCAN_THREADS / WAVE];
    __shared__ uint32_t s_bid;
    __shared__ uint64_t s_excl;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (threadIdx.x == 0) s_bid = atomicAdd(&st->ticket, 1u);
    __syncthreads();
    const uint32_t bid = s_bid;
    const int64_t base = (int64_t)bid * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int64_t i = base + k;
        v[k] = i < n ? (perm ? perm_value(in, perm[i]) : in[i]) : 0u;
        s += v[k];
    }
    uint32_t btotal;
    const uint32_t excl_in_tile = block_exclusive_scan<SCAN_THREADS>(s, wsum, &btotal);
    if (w == 0) {
        uint64_t* mine = st->status + bid;
        uint64_t excl = 0;
        if (bid == 0) {
            if (lane == 0) __hip_atomic_store(mine, (uint64_t)btotal | SC_INCL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(mine, (uint64_t)btotal | SC_LOCAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t pb = (int64_t)bid - 1;
            uint32_t spins = 0;
            bool reported = false;
            while (true) {
                const int64_t idx = pb - lane;
                const uint64_t word = idx >= 0 ? __hip_atomic_load(st->status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                               : SC_INCL;  // before tile 0: inclusive prefix 0
                const uint64_t flag = word & ~SC_VAL;
                const uint64_t ready = __builtin_amdgcn_ballot_w64(flag != 0);
                const uint64_t has_incl = __builtin_amdgcn_ballot_w64(flag == SC_INCL);
                const int first = has_incl ? __builtin_ctzll(has_incl) : WAVE - 1;   // nearest inclusive prefix
                const uint64_t need = first == WAVE - 1 ? ~0ull : ((1ull << (first + 1)) - 1ull);
                if ((ready & need) != need) {
                    if (++spins > g_spin_limit && !reported) { reported = true; if (lane == 0) lookback_timeout(&st->error); }
                    if (spins > SPIN_HARD_LIMIT) __builtin_trap();   // wedged: fault instead of hanging for ever
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                uint64_t part = lane <= first ? (word & SC_VAL) : 0ull;
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) part += __shfl_xor(part, d, WAVE);
                excl += part;
                if (has_incl) break;
                pb -= WAVE;
            }
            if (lane == 0)
                __hip_atomic_store(mine, ((excl + btotal) & SC_VAL) | SC_INCL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_excl = excl;
            if (total && (int64_t)(bid + 1) * SCAN_TILE >= n) *total = excl + btotal;
        }
    }
    __syncthreads();
    uint32_t run = (uint32_t)s_excl + excl_in_tile;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int64_t i = base + k;
        if (EXCLUSIVE) {
            if (i < n) out[i] = run;
            run += v[k];
        } else {
            const uint32_t prev = run;
            run += v[k];
            if (i < n) {
                out[i] = run;
                // element i owns the output range [prev, run): record it as the owner of every
                // multiple of `span` inside (the emit kernel starts its rank search there)
                if (span_owner && run > prev)
                    for (uint32_t b = (prev + span - 1) / span; (uint64_t)b * span < run && b < span_cap; ++b)
                        span_owner[b] = (uint32_t)i;
            }
        }
    }
}

size_t scan_state_bytes(int64_t n)
{
    const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nb > SCAN_ONEPASS_MAX_BLOCKS) return 0;
    return align_up(sizeof(ScanState) + (size_t)(nb > 0 ? nb : 1) * sizeof(uint64_t), 256);
}

// which of the two forms below a scan of n words takes: 0 nothing to do, 1 the one-pass look-back, 2 three kernels
int scan_path(int64_t n) { return n <= 0 ? 0 : (scan_state_bytes(n) ? 1 : 2); }

size_t scan_tmp_bytes(int64_t n)
{
    const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    const size_t three_kernel = align_up((size_t)(nb + 2) * sizeof(uint64_t), 256);
    const size_t one_pass = scan_state_bytes(n);
    return three_kernel > one_pass ? three_kernel : one_pass;
}

template <bool EXCLUSIVE>
static int scan_u32(int64_t n, const uint32_t* in, const uint32_t* perm, uint32_t* out, uint32_t* total,
                    void* tmp, hipStream_t stream)
{
    uint64_t* partial = reinterpret_cast<uint64_t*>(tmp);
    if (n <= 0) {
        if (total) SR_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(uint64_t), stream));
        return SPLATRASTER_OK;
    }
    const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, stream, n, in, perm, partial);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(1024), 0, stream, nb, partial,
                       reinterpret_cast<uint64_t*>(total));
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_apply_kernel<EXCLUSIVE>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, stream, n, in,
                       perm, partial, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int inclusive_scan_u32(int64_t n, const uint32_t* in, const uint32_t* perm, uint32_t* out, uint32_t* total,
                       void* tmp, hipStream_t stream, bool state_zeroed, uint32_t* span_owner, uint32_t span,
                       uint32_t span_cap)
{
    const size_t state = scan_state_bytes(n);
    if (n > 0 && state) {
        if (!state_zeroed) SR_HIP_CHECK(hipMemsetAsync(tmp, 0, state, stream));
        const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
        hipLaunchKernelGGL(scan_onepass_kernel<false>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, stream, n, in, perm, out,
                           reinterpret_cast<uint64_t*>(total), reinterpret_cast<ScanState*>(tmp), span_owner, span, span_cap);
        SR_LAUNCH_CHECK();
        return SPLATRASTER_OK;
    }
    return scan_u32<false>(n, in, perm, out, total, tmp, stream);
}

int exclusive_scan_u32(int64_t n, uint32_t* inout, uint32_t* total, void* tmp, hipStream_t stream, bool state_zeroed)
{
    const size_t state = scan_state_bytes(n);
    if (n > 0 && state) {
        if (!state_zeroed) SR_HIP_CHECK(hipMemsetAsync(tmp, 0, state, stream));
        const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
        hipLaunchKernelGGL(scan_onepass_kernel<true>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, stream, n, inout, nullptr, inout,
                           reinterpret_cast<uint64_t*>(total), reinterpret_cast<ScanState*>(tmp), nullptr, 0u, 0u);
        SR_LAUNCH_CHECK();
        return SPLATRASTER_OK;
    }
    return scan_u32<true>(n, inout, nullptr, inout, total, tmp, stream);
}

// ---------------------------------------------------------------------------------------
// radix sort
// ---------------------------------------------------------------------------------------
// KIn / KOut: the key type a pass reads / writes.  uint32_t everywhere but in the tile sort of a window whose (view, tile)
// ids fit 16 bits (sort_pairs_k16 below): there every pass reads uint16_t keys and only the last one widens them.
template <typename KIn>
__global__ void __launch_bounds__(SORT_THREADS)
sort_hist_kernel(int64_t n, const KIn* __restrict__ keys, int shift, uint32_t nblocks,
                 uint32_t* __restrict__ table, uint32_t* __restrict__ zero, uint32_t nzero)
{
    __shared__ uint32_t hist[RADIX];
    // look-back state of the one-pass scan that follows: cleared here, not by a memset launch
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < nzero; w += gridDim.x * blockDim.x) zero[w] = 0u;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; ++k) {
        const int64_t i = base + (int64_t)k * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[((uint32_t)keys[i] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * nblocks + blockIdx.x] = hist[threadIdx.x];
}

// ---- the three steps that both scatter kernels share; a wave owns the ITEMS * WAVE keys from wbase on, lane l those at k * WAVE + l ----
template <int ITEMS, typename KIn>
__device__ __forceinline__ void sort_load(int64_t n, int64_t wbase, const KIn* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                          uint32_t (&key)[ITEMS], uint32_t (&val)[ITEMS])
{
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * WAVE + lane;
        const bool valid = i < n;
        key[k] = valid ? (uint32_t)keys_in[i] : 0u;
        val[k] = valid ? vals_in[i] : 0u;
    }
}

// rank[k]: the keys of this wave with key k's digit that come before it; hist (this wave's 256 zeroed counters) ends as the counts
template <int ITEMS>
__device__ __forceinline__ void sort_rank(int64_t n, int64_t wbase, int shift, const uint32_t (&key)[ITEMS], uint32_t* hist,
                                          uint32_t (&rank)[ITEMS])
{
    const int lane = threadIdx.x & (WAVE - 1);
    const uint64_t lt_mask = lanes_below(lane);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * WAVE + lane;
        const bool valid = i < n;
        const uint32_t digit = (key[k] >> shift) & (RADIX - 1);
        uint64_t mask = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            mask &= bit ? bal : ~bal;
        }
        uint32_t prev = 0;
        if (valid) prev = hist[digit];
        rank[k] = prev + (uint32_t)__popcll(mask & lt_mask);
        // lowest lane of each equal-digit group publishes the new count
        if (valid && (mask & lt_mask) == 0) hist[digit] = prev + (uint32_t)__popcll(mask);
    }
}

// thread d: the per-wave counts of digit d become the bases of (wave k, digit d), from `run` on
__device__ __forceinline__ void sort_bases(uint32_t (&wave_hist)[SORT_WAVES][RADIX], int d, uint32_t run)
{
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) {
        const uint32_t c = wave_hist[k][d];
        wave_hist[k][d] = run;
        run += c;
    }
}

template <typename KIn, typename KOut>
__global__ void __launch_bounds__(SORT_THREADS)
sort_scatter_kernel(int64_t n, const KIn* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                    KOut* __restrict__ keys_out, uint32_t* __restrict__ vals_out, int shift,
                    uint32_t nblocks, const uint32_t* __restrict__ table)
{
    __shared__ uint32_t wave_hist[SORT_WAVES][RADIX];
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) wave_hist[k][threadIdx.x] = 0;
    __syncthreads();

    const int64_t wbase = (int64_t)blockIdx.x * SORT_TILE + (int64_t)w * (SORT_ITEMS * WAVE);
    uint32_t key[SORT_ITEMS], val[SORT_ITEMS], rank[SORT_ITEMS];
    sort_load(n, wbase, keys_in, vals_in, key, val);
    sort_rank(n, wbase, shift, key, wave_hist[w], rank);
    __syncthreads();
    // Block-local reorder through LDS before the global scatter: elements of one digit become
    // consecutive, so consecutive threads write consecutive addresses (runs of ~16 elements at
    // 256 bins) instead of 64 scattered 4-byte stores per instruction.
    __shared__ KIn s_keys[SORT_TILE];
    __shared__ uint32_t s_vals[SORT_TILE];
    __shared__ uint32_t s_gbase[RADIX];   // global address of local slot 0 of the digit's run
    __shared__ uint32_t s_wsum[SORT_WAVES];
    {
        const int d = threadIdx.x;
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < SORT_WAVES; ++k) total += wave_hist[k][d];
        // exclusive prefix of `total` over the 256 digits
        const uint32_t excl = block_exclusive_scan<SORT_THREADS>(total, s_wsum);
        s_gbase[d] = table[(size_t)d * nblocks + blockIdx.x] - excl;
        sort_bases(wave_hist, d, excl);   // block-local bases
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * WAVE + lane;
        if (i < n) {
            const uint32_t digit = (key[k] >> shift) & (RADIX - 1);
            const uint32_t pos = wave_hist[w][digit] + rank[k];
            s_keys[pos] = (KIn)key[k];
            s_vals[pos] = val[k];
        }
    }
    __syncthreads();
    const int64_t bbase = (int64_t)blockIdx.x * SORT_TILE;
    const uint32_t cnt = (uint32_t)((n - bbase) < (int64_t)SORT_TILE ? (n - bbase) : (int64_t)SORT_TILE);
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; ++k) {
        const uint32_t sl = (uint32_t)k * SORT_THREADS + threadIdx.x;
        if (sl < cnt) {
            const uint32_t kk = s_keys[sl];
            const uint32_t dst = s_gbase[(kk >> shift) & (RADIX - 1)] + sl;
            keys_out[dst] = (KOut)kk;
            vals_out[dst] = s_vals[sl];
        }
    }
}

// ---------------------------------------------------------------------------------------
// one-sweep passes: ONE histogram kernel for every digit position, then ONE kernel per pass
// that ranks, resolves its global offsets with a decoupled look-back over the preceding
// blocks, and scatters.  21 -> 7 launches for the 32-bit depth sort, 10 -> 4 for the tile sort.
//
// Look-back protocol (MI355X_MICROARCH.md, inter-workgroup visibility): one 32-bit status
// word per (block, digit) = count | flag (1 = block-local count, 2 = inclusive prefix),
// written once per state with a relaxed AGENT-scope atomic store and polled with relaxed
// agent-scope atomic loads — the data IS the flag, so no fence is needed.  Blocks take their
// logical index from an atomic ticket, so a block only ever waits for blocks that have
// already started: no residency assumption, no deadlock.  A block that waits longer than the spin
// bound raises the host-visible watchdog flag (lookback_timeout above) and goes on waiting.
// ---------------------------------------------------------------------------------------
constexpr uint32_t ST_LOCAL = 1u << 30, ST_INCL = 2u << 30, ST_MASK = (1u << 30) - 1u;
constexpr int MAX_PASSES = 4;

struct SweepState {        // all zeroed by one memset before the passes
    uint32_t totals[MAX_PASSES][RADIX];
    uint32_t ticket[MAX_PASSES];
    uint32_t error;
    uint32_t pad[3];
};

// ITEMS keys per thread: the one-sweep kernels are latency-bound chains per block, so a sort of P = 500 k keys
// in 4096-key tiles (123 blocks) leaves half of the 256 CUs idle; with 2048-key tiles every CU has a block
// and each block's chain is half as long (sweep_items below picks the tile)
template <int ITEMS>
__global__ void __launch_bounds__(SORT_THREADS)
sort_hist_all_kernel(int64_t n, const uint32_t* __restrict__ keys, int passes, SweepState* __restrict__ st)
{
    __shared__ uint32_t hist[MAX_PASSES][RADIX];
#pragma unroll
    for (int p = 0; p < MAX_PASSES; ++p) hist[p][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (SORT_THREADS * ITEMS);
#pragma unroll 4
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = base + (int64_t)k * SORT_THREADS + threadIdx.x;
        if (i < n) {
            const uint32_t key = keys[i];
            for (int p = 0; p < passes; ++p) atomicAdd(&hist[p][(key >> (8 * p)) & (RADIX - 1)], 1u);
        }
    }
    __syncthreads();
    for (int p = 0; p < passes; ++p) {
        const uint32_t c = hist[p][threadIdx.x];
        if (c) atomicAdd(&st->totals[p][threadIdx.x], c);
    }
}

template <int ITEMS>
__global__ void __launch_bounds__(SORT_THREADS)
sort_sweep_kernel(int64_t n, const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                  uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out, int pass,
                  SweepState* __restrict__ st, uint32_t* __restrict__ status /*[nblocks][RADIX], zeroed*/)
{
    __shared__ uint32_t wave_hist[SORT_WAVES][RADIX];
    __shared__ uint32_t s_scan[SORT_WAVES];
    __shared__ uint32_t s_bid;
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int shift = 8 * pass;
    if (threadIdx.x == 0) s_bid = atomicAdd(&st->ticket[pass], 1u);
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) wave_hist[k][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t bid = s_bid;

    const int64_t wbase = (int64_t)bid * (SORT_THREADS * ITEMS) + (int64_t)w * (ITEMS * WAVE);
    uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
    sort_load(n, wbase, keys_in, vals_in, key, val);
    sort_rank(n, wbase, shift, key, wave_hist[w], rank);
    __syncthreads();
    {
        const int d = threadIdx.x;
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < SORT_WAVES; ++k) cnt += wave_hist[k][d];
        uint32_t* mine = status + (size_t)bid * RADIX + d;
        // publish, then look back over the preceding blocks
        uint32_t excl = 0;
        if (bid == 0) {
            __hip_atomic_store(mine, cnt | ST_INCL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            __hip_atomic_store(mine, cnt | ST_LOCAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // LOOKBACK independent loads in flight per step: the walk over predecessors that have
            // only published their local count costs one L2 round trip per LOOKBACK blocks
            constexpr int LOOKBACK = SR_SORT_LOOKBACK;
            int64_t pb = (int64_t)bid - 1;
            uint32_t spins = 0;
            bool done = false, reported = false;
            while (pb >= 0 && !done) {
                uint32_t v[LOOKBACK];
#pragma unroll
                for (int q = 0; q < LOOKBACK; ++q) {
                    const int64_t idx = pb - q;
                    v[q] = idx >= 0 ? __hip_atomic_load(status + (size_t)idx * RADIX + d, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT)
                                    : ST_INCL;  // before block 0: inclusive prefix 0
                }
                int used = 0;
#pragma unroll
                for (int q = 0; q < LOOKBACK; ++q) {
                    if (done || used != q) continue;
                    const uint32_t flag = v[q] & ~ST_MASK;
                    if (flag == 0) continue;  // not published yet: retry from here
                    excl += v[q] & ST_MASK;
                    used = q + 1;
                    if (flag == ST_INCL) done = true;
                }
                pb -= used;
                if (used == 0) {
                    if (++spins > g_spin_limit && !reported) { reported = true; lookback_timeout(&st->error); }
                    if (spins > SPIN_HARD_LIMIT) __builtin_trap();   // wedged: fault instead of hanging for ever
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            __hip_atomic_store(mine, (excl + cnt) | ST_INCL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // exclusive scan of the digit totals across the 256 threads -> global base of digit d
        const uint32_t tot = st->totals[pass][d];
        sort_bases(wave_hist, d, block_exclusive_scan<SORT_THREADS>(tot, s_scan) + excl);   // global bases
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * WAVE + lane;
        if (i < n) {
            const uint32_t digit = (key[k] >> shift) & (RADIX - 1);
            const uint32_t dst = wave_hist[w][digit] + rank[k];
            keys_out[dst] = key[k];
            vals_out[dst] = val[k];
        }
    }
}

#ifndef SR_SORT_ONESWEEP
#define SR_SORT_ONESWEEP 1  // 0 = histogram / scan / scatter kernels per pass (A/B baseline)
#endif

// keys per thread of the one-sweep path (0: the sort takes the histogram / scan / scatter passes instead)
static int sweep_items(int64_t n)
{
    if (!SR_SORT_ONESWEEP || n <= 0) return 0;
    if (n <= (int64_t)256 * SORT_THREADS * 8) return 8;            // <= 524 288 keys: 2048-key tiles, <= 256 blocks
    if (n <= (int64_t)256 * SORT_TILE) return SORT_ITEMS;          // <= 1 048 576 keys: 4096-key tiles
    return 0;
}
static int64_t sweep_blocks(int64_t n)
{
    const int64_t tile = (int64_t)SORT_THREADS * sweep_items(n);
    return tile ? (n + tile - 1) / tile : 0;
}

// words of the [digit][block] table that every histogram / scan / scatter pass scans
static int64_t sort_table_words(int64_t nb) { return nb * RADIX; }

// The sort's scratch in its two forms (base null: `bytes` only).  One-sweep: [SweepState | one status table per pass].
struct SweepLayout { SweepState* st; uint32_t* status[MAX_PASSES]; size_t bytes; };
static SweepLayout sweep_layout(void* tmp, int64_t n, int passes)
{
    const int64_t nbs = sweep_blocks(n);
    SweepLayout L{};
    Carver c{tmp};
    L.st = c.take<SweepState>(1);
    for (int p = 0; p < passes; ++p) L.status[p] = c.take<uint32_t>((size_t)(nbs > 0 ? nbs : 1) * RADIX);
    L.bytes = c.o;
    return L;
}
// Histogram passes over nb blocks: [table | state of the table's scan].
struct HistLayout { uint32_t* table; void* scan_tmp; size_t bytes; };
static HistLayout hist_layout(void* tmp, int64_t nb)
{
    HistLayout L;
    Carver c{tmp};
    L.table = c.take<uint32_t>((size_t)sort_table_words(nb));
    L.scan_tmp = c.take<char>(scan_tmp_bytes(sort_table_words(nb)));
    L.bytes = c.o;
    return L;
}

size_t sort_tmp_bytes(int64_t n)
{
    const int64_t nb = (n + SORT_TILE - 1) / SORT_TILE;
    const size_t hist = hist_layout(nullptr, nb > 0 ? nb : 1).bytes, sweep = sweep_layout(nullptr, n, MAX_PASSES).bytes;
    return hist > sweep ? hist : sweep;
}

// bytes at the start of tmp that must be zero before sort_pairs_u32 (0: none); a caller that
// zeroes them itself passes tmp_zeroed = true
size_t sort_zero_bytes(int64_t n, int key_bits)
{
    if (n <= 0 || key_bits <= 0 || !sweep_items(n)) return 0;
    return sweep_layout(nullptr, n, (key_bits + 7) / 8).bytes;
}

// histogram / scan / scatter passes over 8-bit digits, ping-ponging between (kin, vin) and (kout, vout).  KIn = uint16_t:
// the key arrays hold uint16_t (in the first half of their uint32_t storage) up to the input of the last pass, which
// writes uint32_t keys — a pass never reads and writes the same buffer, so the two widths cannot overlap.

template <typename KIn>
static int sort_passes(int64_t n, int64_t nb, int passes, uint32_t* kin, uint32_t* vin, uint32_t* kout, uint32_t* vout, void* tmp,
                       hipStream_t stream, bool* result_in_alt)
{
    const HistLayout L = hist_layout(tmp, nb);
    uint32_t* table = L.table;
    void* scan_tmp = L.scan_tmp;
    for (int p = 0; p < passes; ++p) {
        const int shift = p * 8;
        const int64_t cnt = sort_table_words(nb);
        const size_t sstate = scan_state_bytes(cnt);
        hipLaunchKernelGGL(sort_hist_kernel<KIn>, dim3((unsigned)nb), dim3(SORT_THREADS), 0, stream, n,
                           reinterpret_cast<const KIn*>(kin), shift, (uint32_t)nb, table, reinterpret_cast<uint32_t*>(scan_tmp),
                           (uint32_t)(sstate / 4));
        SR_LAUNCH_CHECK();
        if (sstate) {
            const int64_t snb = (cnt + SCAN_TILE - 1) / SCAN_TILE;
            hipLaunchKernelGGL(scan_onepass_kernel<true>, dim3((unsigned)snb), dim3(SCAN_THREADS), 0, stream, cnt, table,
                               nullptr, table, nullptr, reinterpret_cast<ScanState*>(scan_tmp), nullptr, 0u, 0u);
            SR_LAUNCH_CHECK();
        } else {
            int st = scan_u32<true>(cnt, table, nullptr, table, nullptr, scan_tmp, stream);
            if (st != SPLATRASTER_OK) return st;
        }
        if (p + 1 < passes)
            hipLaunchKernelGGL((sort_scatter_kernel<KIn, KIn>), dim3((unsigned)nb), dim3(SORT_THREADS), 0, stream, n,
                               reinterpret_cast<const KIn*>(kin), vin, reinterpret_cast<KIn*>(kout), vout, shift, (uint32_t)nb, table);
        else
            hipLaunchKernelGGL((sort_scatter_kernel<KIn, uint32_t>), dim3((unsigned)nb), dim3(SORT_THREADS), 0, stream, n,
                               reinterpret_cast<const KIn*>(kin), vin, kout, vout, shift, (uint32_t)nb, table);
        SR_LAUNCH_CHECK();
        uint32_t* t = kin; kin = kout; kout = t;
        t = vin; vin = vout; vout = t;
    }
    *result_in_alt = (passes & 1) != 0;
    return SPLATRASTER_OK;
}

int sort_pairs_u32(int64_t n, uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt,
                   int key_bits, void* tmp, hipStream_t stream, bool* result_in_alt, bool tmp_zeroed)
{
    *result_in_alt = false;
    if (n <= 0 || key_bits <= 0) return SPLATRASTER_OK;
    if (n >= (int64_t)1 << 32) return SPLATRASTER_ERR_OVERFLOW;
    const int64_t nb = (n + SORT_TILE - 1) / SORT_TILE;
    uint32_t *kin = keys, *vin = vals, *kout = keys_alt, *vout = vals_alt;
    const int passes = (key_bits + 7) / 8;
    // one-sweep for small sorts (launch-latency-bound); the serial look-back of thread d over
    // its predecessors costs more than it saves beyond a few hundred blocks (S2 tile sort:
    // 0.161 vs 0.121 ms with 975 blocks), there the histogram/scan/scatter passes are kept.
    if (sweep_items(n)) {
        const int items = sweep_items(n);
        const int64_t nbs = sweep_blocks(n);
        const SweepLayout L = sweep_layout(tmp, n, passes);
        SweepState* st = L.st;
        if (!tmp_zeroed) SR_HIP_CHECK(hipMemsetAsync(tmp, 0, L.bytes, stream));
        if (items == 8)
            hipLaunchKernelGGL(sort_hist_all_kernel<8>, dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, n, kin, passes, st);
        else
            hipLaunchKernelGGL(sort_hist_all_kernel<SORT_ITEMS>, dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, n, kin, passes, st);
        SR_LAUNCH_CHECK();
        for (int p = 0; p < passes; ++p) {
            uint32_t* status = L.status[p];
            if (items == 8)
                hipLaunchKernelGGL(sort_sweep_kernel<8>, dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, n, kin, vin, kout,
                                   vout, p, st, status);
            else
                hipLaunchKernelGGL(sort_sweep_kernel<SORT_ITEMS>, dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, n, kin, vin,
                                   kout, vout, p, st, status);
            SR_LAUNCH_CHECK();
            uint32_t* t = kin; kin = kout; kout = t;
            t = vin; vin = vout; vout = t;
        }
        *result_in_alt = (passes & 1) != 0;
        return SPLATRASTER_OK;
    }
    return sort_passes<uint32_t>(n, nb, passes, kin, vin, kout, vout, tmp, stream, result_in_alt);
}

// The tile sort of a window: global tile ids of at most 16 bits, written as uint16_t by emit_kernel, when the sort takes
// the histogram / scan / scatter passes (the one-sweep form of small sorts is latency-bound: narrower keys buy nothing there).
bool sort_keys16(int64_t n, int key_bits) { return n > 0 && key_bits > 0 && key_bits <= 16 && !sweep_items(n); }

// sort_pairs_u32 for such keys: keys / keys_alt are the [n] uint32_t arrays of the 32-bit path, an array of uint16_t keys
// lives in the first half of one; the result (the buffer that sort_pairs_u32 would leave it in) holds uint32_t keys.
int sort_pairs_k16(int64_t n, uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, int key_bits, void* tmp,
                   hipStream_t stream, bool* result_in_alt)
{
    *result_in_alt = false;
    if (!sort_keys16(n, key_bits)) return SPLATRASTER_ERR_BAD_ARG;
    if (n >= (int64_t)1 << 32) return SPLATRASTER_ERR_OVERFLOW;
    const int64_t nb = (n + SORT_TILE - 1) / SORT_TILE;
    return sort_passes<uint16_t>(n, nb, (key_bits + 7) / 8, keys, vals, keys_alt, vals_alt, tmp, stream, result_in_alt);
}

// the decisions above, for the tests (splatraster_debug_sort_path): 0 nothing to do, 1 / 2 one-sweep with 2048- / 4096-key
// tiles, 3 histogram / scan / scatter passes, 4 the same on uint16_t keys; +8 when the table scan of a pass takes three kernels
int sort_path(int64_t n, int key_bits, bool keys16)
{
    if (n <= 0 || key_bits <= 0) return 0;
    const int items = sweep_items(n);
    if (items) return items == 8 ? 1 : 2;
    const int64_t nb = (n + SORT_TILE - 1) / SORT_TILE;
    return (keys16 ? 4 : 3) + (scan_path(sort_table_words(nb)) == 2 ? 8 : 0);
}

}  // namespace sr
