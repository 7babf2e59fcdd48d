// retrieval.hip — the two ends of test.py --eval_pose that frame the per-query stages (include/splatraster.h):
//   retrieval_topk   pre_process/gen_netvlad_retrieval.py:32-34  einsum("id,jd->ij") + topk, fused: the Q x N similarity matrix
//                    never exists in global memory
//   pose_errors      utils/eval_utils.py:75-145                  SO3_to_quat, compute_quaternion_dist, eval_pose
//   pose_invert      test.py:81-82                               camera-to-world from the world-to-camera PnP result
#include "common.h"
#include "mfma_tile.h"
#include "scan.h"

namespace sr {

namespace {

constexpr int RT_THREADS = 256;                 // four waves
constexpr int RT_TN = 128;                      // database rows of a step: one 32-row block per wave
constexpr int RT_KC = 32;                       // descriptor entries staged through LDS at a time
constexpr int RT_LD = RT_KC + 4;                // row stride of the staging tiles (float4-aligned, off the bank period)
constexpr int RT_CLD = RT_TN + 4;               // row stride of the 32-row similarity tile that reuses the staging area
constexpr int RT_MAX_K = SPLATRASTER_RETRIEVAL_MAX_K;
constexpr int RT_MAX_SLICES = 64;
constexpr int RT_TARGET_GROUPS = 512;           // two workgroups per CU before the database is split any further
constexpr int RT_WIDE_RB = 4;                   // 128 query rows per workgroup when the problem fills the chip that way ...
constexpr int RT_WIDE_MAX_K = 32;               // ... and the lists of 128 rows stay small
static_assert((32 + RT_TN) * RT_LD >= 32 * RT_CLD, "the similarity tile must fit the staging area");
static_assert(RT_MAX_K == 2 * WAVE, "a wave holds a list in two registers per lane");

// (similarity, index) as one key: a larger key is a larger similarity, then a smaller index.  Never 0 for a real entry.
__device__ __forceinline__ unsigned long long pack_key(float s, uint32_t n)
{
    s += 0.f;   // -0 -> +0: equal similarities must give equal high words
    return ((unsigned long long)float_order_key(s) << 32) | (unsigned long long)(0xFFFFFFFFu - n);
}
__device__ __forceinline__ float key_sim(unsigned long long key) { return float_from_order_key((uint32_t)(key >> 32)); }
__device__ __forceinline__ int64_t key_index(unsigned long long key) { return (int64_t)(0xFFFFFFFFu - (uint32_t)key); }

// A wave's running list: entry j (descending) in l0 of lane j (j < 64) or l1 of lane j - 64; entries from k on stay 0.
// Inserts the candidates `key` of the 64 lanes (0 = none) that beat the list's k-th entry.
__device__ __forceinline__ void wave_insert(unsigned long long& l0, unsigned long long& l1, unsigned long long key, int k, int lane)
{
    const int last = k - 1;
    unsigned long long thr = last < WAVE ? __shfl(l0, last) : __shfl(l1, last - WAVE);
    unsigned long long todo = __ballot(key > thr);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const unsigned long long x = __shfl(key, src);
        if (x <= thr) continue;   // the list has moved on since the ballot
        const int p = __popcll(__ballot(l0 > x)) + __popcll(__ballot(l1 > x));   // entries in front of x
        unsigned long long up0 = __shfl_up(l0, 1), up1 = __shfl_up(l1, 1);
        const unsigned long long wrap = __shfl(l0, WAVE - 1);
        if (lane == 0) up1 = wrap;
        const int j0 = lane, j1 = lane + WAVE;
        l0 = j0 < p ? l0 : (j0 == p ? x : up0);
        l1 = j1 < p ? l1 : (j1 == p ? x : up1);
        if (j0 >= k) l0 = 0;
        if (j1 >= k) l1 = 0;
        thr = last < WAVE ? __shfl(l0, last) : __shfl(l1, last - WAVE);
    }
}

// One workgroup: 32 * RB query rows against the database steps [blockIdx.y * steps_per_slice, ...).  Each wave accumulates RB
// 32 x 32 blocks (query block x its 32 database rows of the step) over D with the exact-f32 MFMA (mfma_tile.h has the layout, the
// chain and the staging, which is the same chain with float4 loads or scalar ones); after a step the similarities
// of one query block at a time go through LDS to the wave that owns the query row (8 rows of the block per wave), which folds
// them into the row's list (dynamic LDS: [32 * RB][k] keys).
// direct: one slice, the lists are final -> idx / sims; else the slice's lists go to `partial` [Q][slices][k].
template <bool VEC, int RB>
__global__ void __launch_bounds__(RT_THREADS)
retrieval_kernel(int64_t Q, int64_t N, int32_t D, int32_t k, const float* __restrict__ query, const float* __restrict__ db,
                 int32_t steps_per_slice, int32_t direct, unsigned long long* __restrict__ partial, int64_t* __restrict__ idx,
                 float* __restrict__ sims, int32_t* __restrict__ status)
{
    constexpr int TQ = 32 * RB;
    using Tile = StackedTile<RT_THREADS, TQ, RT_TN, RT_KC, VEC>;   // query rows above the step's database rows (mfma_tile.h)
    static_assert(Tile::LD == RT_LD, "the similarity tile is sized against this stride");
    __shared__ __attribute__((aligned(16))) float s_stage[Tile::ROWS * RT_LD];
    extern __shared__ unsigned long long s_list[];   // [TQ][k]
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int64_t steps = (N + RT_TN - 1) / RT_TN;
    const int64_t step0 = (int64_t)blockIdx.y * steps_per_slice;
    const int64_t step1 = step0 + steps_per_slice < steps ? step0 + steps_per_slice : steps;
    const int nkc = (D + RT_KC - 1) / RT_KC;
    const int64_t nchunks = (step1 - step0) * nkc;

    for (int i = tid; i < TQ * k; i += RT_THREADS) s_list[i] = 0;

    Tile tile;
    auto fetch = [&](int64_t chunk) {
        tile.fetch(query, q0, Q, db, (step0 + chunk / nkc) * RT_TN, N, D, (int32_t)(chunk % nkc) * RT_KC, tid);
    };
    f32x16 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc_zero(acc[rb]);
    bool nan_seen = false;
    if (nchunks > 0) fetch(0);
#pragma unroll 1
    for (int64_t chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();   // the previous chunk's MFMAs (or the previous step's merge) have read the staging area
        tile.stage(s_stage, tid);
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);   // in flight under the MFMAs
        const float* qa = s_stage + c * RT_LD;
        const float* da = s_stage + (TQ + wave * 32 + c) * RT_LD;
#pragma unroll
        for (int j = 0; j < RT_KC / 4; ++j) {
            const float2 b = pick(*reinterpret_cast<const float4*>(da + 4 * j), half);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                mfma_k4(acc[rb], pick(*reinterpret_cast<const float4*>(qa + rb * 32 * RT_LD + 4 * j), half), b);
        }
        if ((chunk + 1) % nkc != 0) continue;
        // the step is complete: per query block, similarities -> LDS [query row of the block][database row of the step]
        const int64_t n0 = (step0 + chunk / nkc) * RT_TN;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s_stage[acc_row(i, half) * RT_CLD + wave * 32 + c] = acc[rb][i];
                acc[rb][i] = 0.f;
            }
            __syncthreads();
#pragma unroll 1
            for (int rr = 0; rr < 8; ++rr) {
                const int rl = wave * 8 + rr, r = rb * 32 + rl;
                if (q0 + r >= Q) break;
                unsigned long long l0 = lane < k ? s_list[r * k + lane] : 0ull;
                unsigned long long l1 = lane + WAVE < k ? s_list[r * k + lane + WAVE] : 0ull;
#pragma unroll
                for (int h = 0; h < RT_TN / WAVE; ++h) {
                    const int col = h * WAVE + lane;
                    const int64_t n = n0 + col;
                    const float s = s_stage[rl * RT_CLD + col];
                    unsigned long long key = 0;
                    if (n < N) {
                        nan_seen |= s != s;
                        key = pack_key(s, (uint32_t)n);
                    }
                    wave_insert(l0, l1, key, k, lane);
                }
                if (lane < k) s_list[r * k + lane] = l0;
                if (lane + WAVE < k) s_list[r * k + lane + WAVE] = l1;
            }
        }
    }
    if (nan_seen) status[0] = SPLATRASTER_RETRIEVAL_NONFINITE;
    // a wave wrote the lists of its own rows: no barrier between the merge and this read
#pragma unroll 1
    for (int rr = 0; rr < 8 * RB; ++rr) {
        const int r = (rr >> 3) * 32 + wave * 8 + (rr & 7);
        const int64_t q = q0 + r;
        if (q >= Q) continue;
        for (int j = lane; j < k; j += WAVE) {
            const unsigned long long key = s_list[r * k + j];
            if (direct) {
                idx[q * k + j] = key_index(key);
                sims[q * k + j] = key_sim(key);
            } else {
                partial[(q * gridDim.y + blockIdx.y) * k + j] = key;
            }
        }
    }
}

// one wave per query: the top k of the slices' lists (S * k keys, 0 = an empty slot)
__global__ void __launch_bounds__(WAVE)
retrieval_merge_kernel(int64_t Q, int32_t k, int32_t S, const unsigned long long* __restrict__ partial, int64_t* __restrict__ idx,
                       float* __restrict__ sims)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const unsigned long long* src = partial + q * S * k;
    const int total = S * k;
    unsigned long long l0 = 0, l1 = 0;
    for (int base = 0; base < total; base += WAVE) {
        const int j = base + lane;
        wave_insert(l0, l1, j < total ? src[j] : 0ull, k, lane);
    }
    if (lane < k) {
        idx[q * k + lane] = key_index(l0);
        sims[q * k + lane] = key_sim(l0);
    }
    if (lane + WAVE < k) {
        idx[q * k + lane + WAVE] = key_index(l1);
        sims[q * k + lane + WAVE] = key_sim(l1);
    }
}

// eval_utils.py:90-131 for one matrix (row-major), f64, normalised
__device__ __forceinline__ void so3_to_quat(const double* R, double q[4])
{
    const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
    double s;
    if (r22 < 0 && r00 > r11) {
        s = 1.0 + r00 - r11 - r22;
        q[0] = r12 - r21, q[1] = s, q[2] = r01 + r10, q[3] = r20 + r02;
    } else if (r22 < 0) {   // r00 <= r11
        s = 1.0 - r00 + r11 - r22;
        q[0] = r20 - r02, q[1] = r01 + r10, q[2] = s, q[3] = r12 + r21;
    } else if (r00 < -r11) {   // r22 >= 0
        s = 1.0 - r00 - r11 + r22;
        q[0] = r01 - r10, q[1] = r20 + r02, q[2] = r12 + r21, q[3] = s;
    } else {
        s = 1.0 + r00 + r11 + r22;
        q[0] = s, q[1] = r12 - r21, q[2] = r20 - r02, q[3] = r01 - r10;
    }
    const double root = sqrt(s);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = q[i] * 0.5 / root;
    const double nrm = fmax(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12);   // F.normalize
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] /= nrm;
}

__global__ void __launch_bounds__(256)
pose_errors_kernel(int64_t B, const double* __restrict__ R_est, const double* __restrict__ t_est, const double* __restrict__ R_gt,
                   const double* __restrict__ t_gt, const uint8_t* __restrict__ valid, float* __restrict__ theta_deg,
                   double* __restrict__ dist)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (valid && !valid[b]) {
        theta_deg[b] = __uint_as_float(0x7FC00000u);
        dist[b] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    double qg[4], qe[4];
    so3_to_quat(R_gt + 9 * b, qg);
    so3_to_quat(R_est + 9 * b, qe);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) d += (float)qg[i] * (float)qe[i];
    d = fabsf(d);
    const float lim = (float)(1.0 - 1e-7);   // compute_quaternion_dist's eps, compared and stored in f32
    if (d > lim) d = lim;
    theta_deg[b] = 2.f * acosf(d) * 180.f / (float)3.14159265358979323846;
    const double dx = t_est[3 * b] - t_gt[3 * b], dy = t_est[3 * b + 1] - t_gt[3 * b + 1], dz = t_est[3 * b + 2] - t_gt[3 * b + 2];
    dist[b] = sqrt(dx * dx + dy * dy + dz * dz);
}

__global__ void __launch_bounds__(256)
pose_invert_kernel(int64_t B, const double* __restrict__ R, const double* __restrict__ t, double* __restrict__ R_out,
                   double* __restrict__ t_out)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double* r = R + 9 * b;
    const double t0 = t[3 * b], t1 = t[3 * b + 1], t2 = t[3 * b + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R_out[9 * b + 3 * i + j] = r[3 * j + i];
        t_out[3 * b + i] = fma(-r[6 + i], t2, fma(-r[3 + i], t1, -r[i] * t0));
    }
}

struct RetrievalPlan {
    int64_t tiles, steps;
    int32_t rb, slices, steps_per_slice;
};

bool retrieval_args_ok(int64_t Q, int64_t N, int32_t D, int32_t k)
{
    return Q >= 0 && N >= 1 && N < (1ll << 31) && D >= 1 && k >= 1 && k <= RT_MAX_K && k <= N && Q < (1ll << 31) * 32;
}

RetrievalPlan retrieval_plan(int64_t Q, int64_t N, int32_t k)
{
    RetrievalPlan p;
    p.steps = (N + RT_TN - 1) / RT_TN;
    const int64_t wide_tiles = (Q + 32 * RT_WIDE_RB - 1) / (32 * RT_WIDE_RB);
    p.rb = (k <= RT_WIDE_MAX_K && wide_tiles * p.steps >= RT_TARGET_GROUPS) ? RT_WIDE_RB : 1;
    p.tiles = (Q + 32 * p.rb - 1) / (32 * p.rb);
    int64_t want = p.tiles > 0 ? (RT_TARGET_GROUPS + p.tiles - 1) / p.tiles : 1;
    if (want > RT_MAX_SLICES) want = RT_MAX_SLICES;
    if (want > p.steps) want = p.steps;
    if (want < 1) want = 1;
    p.steps_per_slice = (int32_t)((p.steps + want - 1) / want);
    p.slices = (int32_t)((p.steps + p.steps_per_slice - 1) / p.steps_per_slice);
    return p;
}

}  // namespace

}  // namespace sr

using namespace sr;

extern "C" {

size_t splatraster_retrieval_workspace_bytes(int64_t Q, int64_t N, int32_t D, int32_t k)
{
    if (!retrieval_args_ok(Q, N, D, k) || Q == 0) return 0;
    const RetrievalPlan p = retrieval_plan(Q, N, k);
    return p.slices > 1 ? align_up((size_t)Q * p.slices * k * sizeof(unsigned long long), 256) : 0;
}

int splatraster_retrieval_topk(int64_t Q, int64_t N, int32_t D, int32_t k, const float* query, const float* db, int64_t* idx,
                               float* sims, int32_t* status, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!retrieval_args_ok(Q, N, D, k) || !status || !db) return SPLATRASTER_ERR_BAD_ARG;
    if (Q > 0 && (!query || !idx || !sims)) return SPLATRASTER_ERR_BAD_ARG;
    const RetrievalPlan p = retrieval_plan(Q, N, k);
    if (Q > 0 && p.slices > 1 && !workspace) return SPLATRASTER_ERR_BAD_ARG;
    SR_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    if (Q == 0) return SPLATRASTER_OK;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slices);
    const int32_t direct = p.slices == 1;
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(workspace);
    const bool vec = D % 4 == 0 && ((uintptr_t)query | (uintptr_t)db) % 16 == 0;
    const size_t lds = (size_t)32 * p.rb * k * sizeof(unsigned long long);
#define RT_LAUNCH(V, R)                                                                                                       \
    hipLaunchKernelGGL((retrieval_kernel<V, R>), grid, dim3(RT_THREADS), lds, stream, Q, N, D, k, query, db, p.steps_per_slice, \
                       direct, partial, idx, sims, status)
    if (p.rb == RT_WIDE_RB) {
        if (vec) RT_LAUNCH(true, RT_WIDE_RB);
        else RT_LAUNCH(false, RT_WIDE_RB);
    } else {
        if (vec) RT_LAUNCH(true, 1);
        else RT_LAUNCH(false, 1);
    }
#undef RT_LAUNCH
    SR_LAUNCH_CHECK();
    if (!direct) {
        hipLaunchKernelGGL(retrieval_merge_kernel, dim3((unsigned)Q), dim3(WAVE), 0, stream, Q, k, p.slices, partial, idx, sims);
        SR_LAUNCH_CHECK();
    }
    return SPLATRASTER_OK;
}

int splatraster_pose_errors(int64_t B, const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                            const uint8_t* valid, float* theta_deg, double* dist, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (B < 0 || B >= (1ll << 31) * 256) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (!R_est || !t_est || !R_gt || !t_gt || !theta_deg || !dist) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_errors_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, R_est, t_est, R_gt, t_gt, valid,
                       theta_deg, dist);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_pose_invert(int64_t B, const double* R, const double* t, double* R_out, double* t_out, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (B < 0 || B >= (1ll << 31) * 256) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (!R || !t || !R_out || !t_out) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_invert_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, R, t, R_out, t_out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
