// netvlad_head.hip — everything behind NetVLAD's convolution stack (pre_process/gen_netvlad_retrieval.py:66-68, test.py:229-235):
//   assign     per-location L2 normalisation, the D -> K score projection and its softmax (the soft assignment)
//   aggregate  V = a xh^T - centers * sum a (the GEMM form), intra-normalisation, the flattened descriptor's normalisation
//   project    the whitening y = weight x + bias and the last normalisation
// hloc's NetVLAD layer is not part of the reference tree: include/splatraster.h (splatraster_netvlad_*) and INTEGRATION.md §25 hold
// the definitions, which are this project's own.
// Determinism: no float atomics; every sum has an order fixed by the shape alone (a contraction is the exact-f32 MFMA's fmaf chain
// over ascending index, mfma_tile.h, or two such chains added once; a reduction is a fixed tree, reduce.h's wave_sum_f32 among them),
// and a row b of any output never depends on the other rows of the batch.
// Built with -ffp-contract=off: the norms, the softmax and the centre term round operation by operation.
#include "common.h"
#include "mfma_tile.h"
#include "reduce.h"

namespace sr {

namespace {

constexpr int NV_MAX_K = SPLATRASTER_NETVLAD_MAX_K;
constexpr int NV_T = 64;                        // locations of an assign workgroup / of an aggregation step
constexpr int NV_DC = 32;                       // channels staged per assign chunk
constexpr int NV_WLD = NV_DC + 4;               // row stride of the staged score_w tile
constexpr int NV_SLD = NV_T + 1;                // row stride of the score tile
constexpr int NV_ASSIGN_THREADS = 256;          // four waves: (k block, location block)
constexpr int NV_DT = 32;                       // d rows of an aggregation workgroup
constexpr int NV_AGG_THREADS = 256;             // four waves: (block of 32 clusters, half of a step's locations)
constexpr int NV_ALD = NV_T + 4;                // row stride of the staged xh / a tiles (float4-aligned)
constexpr int NV_AGG_ROWS = NV_DT + NV_MAX_K;   // staged rows of a step: xh, then a
constexpr int NV_AGG_PER_THREAD = NV_AGG_ROWS * NV_T / NV_AGG_THREADS;
constexpr int NV_FIN_THREADS = 1024;            // [16 row groups][64 clusters]
constexpr int NV_FIN_ROWS = NV_FIN_THREADS / NV_MAX_K;
constexpr int PJ_THREADS = 256;                 // four waves, 32 weight rows each
constexpr int PJ_OT = 128;                      // weight rows of a projection tile
constexpr int PJ_BT = 32;                       // images that share one pass over the weights: the MFMA's rows
constexpr int PJ_KC = 32;                       // columns staged through LDS at a time
constexpr int PJ_LD = PJ_KC + 4;
constexpr int PJ_SLICE = 2048;                  // columns of a workgroup: 4096 x 32768 is 32 tiles x 16 slices = 2 workgroups per CU
constexpr int PJ_FIN_THREADS = 256;
constexpr float NV_EPS = 1e-12f;
static_assert(NV_MAX_K == 64 && NV_T == 64, "two 32-wide blocks of clusters and of locations");
static_assert(PJ_SLICE % PJ_KC == 0, "whole chunks");

// One workgroup: image b, locations [n0, n0 + NV_T).  Column norms of the [D, NV_T] slab (four interleaved partial sums per
// column, added in ascending order), then s = score_w xh over chunks of NV_DC channels, xh scaled on the way into LDS, then the
// softmax of every location over its K scores.
__global__ void __launch_bounds__(NV_ASSIGN_THREADS)
netvlad_assign_kernel(int32_t D, int32_t K, int32_t N, int32_t steps, const float* __restrict__ features,
                      const float* __restrict__ score_w, const float* __restrict__ score_b, float* __restrict__ assign,
                      float* __restrict__ inv_norm)
{
    __shared__ float s_w[NV_MAX_K * NV_WLD];
    __shared__ float s_x[NV_DC * NV_T];
    __shared__ float s_s[NV_MAX_K * NV_SLD];
    __shared__ float s_part[4][NV_T];
    __shared__ float s_inv[NV_T];
    __shared__ float s_sum[NV_T];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave & 1, nb = wave >> 1;
    const int64_t b = blockIdx.x / steps;
    const int n0 = (int)(blockIdx.x % steps) * NV_T;
    const float* x = features + b * D * (int64_t)N;

    {
        const int n = n0 + lane;
        float ss = 0.f;
        if (n < N)
            for (int d = wave; d < D; d += 4) {
                const float v = x[(int64_t)d * N + n];
                ss += v * v;
            }
        s_part[wave][lane] = ss;
    }
    __syncthreads();
    if (tid < NV_T) {
        const float ss = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
        const float inv = 1.0f / fmaxf(sqrtf(ss), NV_EPS);
        s_inv[tid] = inv;
        if (n0 + tid < N) inv_norm[b * N + n0 + tid] = inv;
    }

    f32x16 acc;
    acc_zero(acc);
#pragma unroll 1
    for (int d0 = 0; d0 < D; d0 += NV_DC) {
        __syncthreads();   // s_inv is written; the previous chunk's MFMAs have read the tiles
#pragma unroll
        for (int i = 0; i < NV_MAX_K * NV_DC / NV_ASSIGN_THREADS; ++i) {
            const int e = tid + NV_ASSIGN_THREADS * i, k = e >> 5, d = d0 + (e & 31);
            s_w[k * NV_WLD + (e & 31)] = (k < K && d < D) ? score_w[(int64_t)k * D + d] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NV_DC * NV_T / NV_ASSIGN_THREADS; ++i) {
            const int e = tid + NV_ASSIGN_THREADS * i, d = d0 + (e >> 6), n = n0 + (e & 63);
            s_x[e] = (d < D && n < N) ? x[(int64_t)d * N + n] * s_inv[e & 63] : 0.f;
        }
        __syncthreads();
        if (kb * 32 < K) {
            const float* wa = s_w + (kb * 32 + c) * NV_WLD + half;
            const float* xa = s_x + half * NV_T + nb * 32 + c;
#pragma unroll
            for (int j = 0; j < NV_DC / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * j], xa[2 * j * NV_T], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) s_s[(kb * 32 + acc_row(i, half)) * NV_SLD + nb * 32 + c] = acc[i];
    __syncthreads();
    if (tid < NV_T) {   // one location per thread: max, expf, the sum in ascending k
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) {
            const float s = score_b ? s_s[k * NV_SLD + tid] + score_b[k] : s_s[k * NV_SLD + tid];
            s_s[k * NV_SLD + tid] = s;
            m = fmaxf(m, s);
        }
        float sum = 0.f;
        for (int k = 0; k < K; ++k) {
            const float e = expf(s_s[k * NV_SLD + tid] - m);
            s_s[k * NV_SLD + tid] = e;
            sum += e;
        }
        s_sum[tid] = sum;
    }
    __syncthreads();
    float* out = assign + b * K * (int64_t)N;
    for (int e = tid; e < K * NV_T; e += NV_ASSIGN_THREADS) {
        const int k = e >> 6, n = n0 + (e & 63);
        if (n < N) out[(int64_t)k * N + n] = s_s[k * NV_SLD + (e & 63)] / s_sum[e & 63];
    }
}

// One workgroup: image b, rows [d0, d0 + NV_DT) of S = sum_n xh[d, n] a[k, n], walking all N in steps of NV_T in order, so no
// partial sums leave the workgroup.  Wave (kb, nh) holds the block of 32 clusters kb over the locations [32 nh, 32 nh + 32) of
// every step: one fmaf chain over ascending n per element and half; the two halves are added once, at the end, first + second.
// Writes S to v[b, d * K + k].
__global__ void __launch_bounds__(NV_AGG_THREADS)
netvlad_aggregate_kernel(int32_t D, int32_t K, int32_t N, int32_t dblocks, const float* __restrict__ features,
                         const float* __restrict__ assign, const float* __restrict__ inv_norm, float* __restrict__ v)
{
    __shared__ __attribute__((aligned(16))) float s_t[NV_AGG_ROWS * NV_ALD];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave & 1, nh = wave >> 1;
    const int64_t b = blockIdx.x / dblocks;
    const int d0 = (int)(blockIdx.x % dblocks) * NV_DT;
    const float* x = features + b * D * (int64_t)N;
    const float* a = assign + b * K * (int64_t)N;
    const float* inv = inv_norm + b * N;
    const int steps = (N + NV_T - 1) / NV_T;

    float r[NV_AGG_PER_THREAD];
    // staged element of a step: row = wave + 4 i (xh rows first, then a rows), column = lane; zero beyond N.  Rows beyond D and K
    // read the last valid row instead: they only reach accumulator rows and columns that are never stored.
    auto fetch = [&](int step) {
        const int n = step * NV_T + lane;
        const bool live = n < N;
        const float iv = live ? inv[n] : 0.f;
#pragma unroll
        for (int i = 0; i < NV_DT / 4; ++i) {
            const int d = min(d0 + wave + 4 * i, D - 1);
            r[i] = live ? x[(int64_t)d * N + n] * iv : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NV_MAX_K / 4; ++i) {
            const int k = min(wave + 4 * i, K - 1);
            r[NV_DT / 4 + i] = live ? a[(int64_t)k * N + n] : 0.f;
        }
    };

    f32x16 acc;
    acc_zero(acc);
    fetch(0);
#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
        __syncthreads();   // the previous step's MFMAs have read the tiles
#pragma unroll
        for (int i = 0; i < NV_AGG_PER_THREAD; ++i) s_t[(wave + 4 * i) * NV_ALD + lane] = r[i];
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);   // in flight under the MFMAs
        if (kb * 32 < K) {
            const float* xa = s_t + c * NV_ALD + nh * 32;
            const float* aa = s_t + (NV_DT + kb * 32 + c) * NV_ALD + nh * 32;
#pragma unroll
            for (int j = 0; j < NV_T / 8; ++j)
                mfma_k4(acc, pick(*reinterpret_cast<const float4*>(xa + 4 * j), half), pick(*reinterpret_cast<const float4*>(aa + 4 * j), half));
        }
    }
    __syncthreads();   // the tiles are free: the second halves travel through them, [kb][register][lane]
    if (nh == 1)
#pragma unroll
        for (int i = 0; i < 16; ++i) s_t[(kb * 16 + i) * WAVE + lane] = acc[i];
    __syncthreads();
    const int k = kb * 32 + c;
    if (nh == 0 && k < K) {
        float* out = v + b * D * (int64_t)K;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int d = d0 + acc_row(i, half);
            if (d < D) out[(int64_t)d * K + k] = acc[i] + s_t[(kb * 16 + i) * WAVE + lane];
        }
    }
}

// the K sums of s_col[NV_FIN_ROWS][NV_MAX_K] in ascending row order -> s_tot[k]; all threads call
__device__ __forceinline__ void fin_columns(float mine, bool active, int r, int k, int K, float (&s_col)[NV_FIN_ROWS][NV_MAX_K],
                                            float (&s_tot)[NV_MAX_K])
{
    __syncthreads();   // earlier readers of s_col and s_tot are done
    s_col[r][k] = active ? mine : 0.f;
    __syncthreads();
    if (r == 0 && k < K) {
        float t = 0.f;
        for (int i = 0; i < NV_FIN_ROWS; ++i) t += s_col[i][k];
        s_tot[k] = t;
    }
    __syncthreads();
}

// One workgroup per image: sum_n a[k, n] (a wave per cluster: 64 interleaved partial sums, then the butterfly), the centre term,
// then the two normalisations.  Thread (r, k) owns the elements d = r, r + 16, ... of column k in every pass, so it only ever
// reads back its own stores.
__global__ void __launch_bounds__(NV_FIN_THREADS)
netvlad_finish_kernel(int32_t D, int32_t K, int32_t N, const float* __restrict__ assign, const float* __restrict__ centers,
                      int32_t flags, float* __restrict__ v)
{
    __shared__ float s_sa[NV_MAX_K];
    __shared__ float s_col[NV_FIN_ROWS][NV_MAX_K];
    __shared__ float s_tot[NV_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, r = tid >> 6, k = lane;
    const int64_t b = blockIdx.x;
    const float* a = assign + b * K * (int64_t)N;
    float* out = v + b * D * (int64_t)K;
    for (int kk = r; kk < K; kk += NV_FIN_ROWS) {
        float p = 0.f;
        for (int n = lane; n < N; n += WAVE) p += a[(int64_t)kk * N + n];
        p = wave_sum_f32(p);
        if (lane == 0) s_sa[kk] = p;
    }
    __syncthreads();
    const bool active = k < K;
    float ss = 0.f;
    if (active) {
        const float sa = s_sa[k];
        for (int d = r; d < D; d += NV_FIN_ROWS) {
            const int64_t i = (int64_t)d * K + k;
            const float t = out[i] - centers[i] * sa;
            out[i] = t;
            ss += t * t;
        }
    }
    if (!(flags & (SPLATRASTER_NETVLAD_INTRANORM | SPLATRASTER_NETVLAD_L2NORM))) return;
    if (flags & SPLATRASTER_NETVLAD_INTRANORM) {
        fin_columns(ss, active, r, k, K, s_col, s_tot);
        ss = 0.f;
        if (active) {
            const float nrm = fmaxf(sqrtf(s_tot[k]), NV_EPS);
            for (int d = r; d < D; d += NV_FIN_ROWS) {
                const int64_t i = (int64_t)d * K + k;
                const float t = out[i] / nrm;
                out[i] = t;
                ss += t * t;
            }
        }
    }
    if (flags & SPLATRASTER_NETVLAD_L2NORM) {
        fin_columns(ss, active, r, k, K, s_col, s_tot);
        float total = 0.f;
        for (int i = 0; i < K; ++i) total += s_tot[i];
        const float nrm = fmaxf(sqrtf(total), NV_EPS);
        if (active)
            for (int d = r; d < D; d += NV_FIN_ROWS) {
                const int64_t i = (int64_t)d * K + k;
                out[i] = out[i] / nrm;
            }
    }
}

// One workgroup: PJ_OT weight rows x the columns [slice * PJ_SLICE, ...) x the PJ_BT images of a batch chunk.  The weights
// stream through LDS once, PJ_KC columns at a time (the next chunk's loads in flight under the MFMAs); each wave accumulates
// [32 images] x [its 32 rows] as one fmaf chain per element over ascending column.  The slice's sums go to
// partial[slice][b][o].
template <bool VEC>
__global__ void __launch_bounds__(PJ_THREADS)
netvlad_project_kernel(int32_t B, int32_t O, int64_t I, int32_t otiles, int32_t slices, const float* __restrict__ x,
                       const float* __restrict__ weight, float* __restrict__ partial)
{
    using Tile = StackedTile<PJ_THREADS, PJ_BT, PJ_OT, PJ_KC, VEC>;   // image rows above the tile's weight rows (mfma_tile.h)
    static_assert(Tile::LD == PJ_LD, "the staging area is declared with this stride");
    __shared__ __attribute__((aligned(16))) float s_stage[Tile::ROWS * PJ_LD];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ot = blockIdx.x % otiles, slice = (blockIdx.x / otiles) % slices, bc = blockIdx.x / otiles / slices;
    const int o0 = ot * PJ_OT, b0 = bc * PJ_BT;
    const int64_t i0 = (int64_t)slice * PJ_SLICE;
    const int64_t i1 = i0 + PJ_SLICE < I ? i0 + PJ_SLICE : I;
    const int nchunks = (int)((i1 - i0 + PJ_KC - 1) / PJ_KC);

    Tile tile;
    auto fetch = [&](int chunk) { tile.fetch(x, b0, B, weight, o0, O, I, i0 + (int64_t)chunk * PJ_KC, tid); };

    f32x16 acc;
    acc_zero(acc);
    fetch(0);
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();   // the previous chunk's MFMAs have read the staging area
        tile.stage(s_stage, tid);
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);   // in flight under the MFMAs
        const float* xa = s_stage + c * PJ_LD;
        const float* wa = s_stage + (PJ_BT + wave * 32 + c) * PJ_LD;
#pragma unroll
        for (int j = 0; j < PJ_KC / 4; ++j)
            mfma_k4(acc, pick(*reinterpret_cast<const float4*>(xa + 4 * j), half), pick(*reinterpret_cast<const float4*>(wa + 4 * j), half));
    }
    const int o = o0 + wave * 32 + c;
    if (o < O) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = b0 + acc_row(i, half);
            if (b < B) partial[((int64_t)slice * B + b) * O + o] = acc[i];
        }
    }
}

// One workgroup per image: the slices' sums in ascending slice order, then the bias, then the normalisation (each wave's
// butterfly, the waves in ascending order).  A thread reads back only its own stores.
__global__ void __launch_bounds__(PJ_FIN_THREADS)
netvlad_project_finish_kernel(int32_t B, int32_t O, int32_t slices, const float* __restrict__ partial,
                              const float* __restrict__ bias, int32_t flags, float* __restrict__ y)
{
    __shared__ float s_red[PJ_FIN_THREADS / WAVE];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float* out = y + b * O;
    float ss = 0.f;
    for (int o = tid; o < O; o += PJ_FIN_THREADS) {
        float t = partial[b * O + o];
        for (int s = 1; s < slices; ++s) t += partial[((int64_t)s * B + b) * O + o];
        if (bias) t += bias[o];
        out[o] = t;
        ss += t * t;
    }
    if (!(flags & SPLATRASTER_NETVLAD_L2NORM)) return;
    ss = wave_sum_f32(ss);
    if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE] = ss;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int w = 0; w < PJ_FIN_THREADS / WAVE; ++w) total += s_red[w];
    const float nrm = fmaxf(sqrtf(total), NV_EPS);
    for (int o = tid; o < O; o += PJ_FIN_THREADS) out[o] = out[o] / nrm;
}

constexpr int64_t NV_GRID_MAX = (1ll << 31) - 1;

bool nv_shape_ok(int32_t B, int32_t D, int32_t K, int32_t N)
{
    if (B < 0 || D < 1 || K < 1 || K > NV_MAX_K || N < 1 || (int64_t)D * K >= (1ll << 31)) return false;
    const int64_t steps = ((int64_t)N + NV_T - 1) / NV_T, dblocks = ((int64_t)D + NV_DT - 1) / NV_DT;
    return B * steps <= NV_GRID_MAX && B * dblocks <= NV_GRID_MAX;   // one workgroup per (image, step) / (image, d block)
}

struct PjPlan {
    int64_t otiles, slices, bchunks, groups;
};

bool pj_shape_ok(int32_t B, int32_t O, int64_t I, PjPlan* p)
{
    if (B < 0 || O < 1 || I < 1 || I >= (1ll << 40)) return false;
    p->otiles = ((int64_t)O + PJ_OT - 1) / PJ_OT;
    p->slices = (I + PJ_SLICE - 1) / PJ_SLICE;
    p->bchunks = ((int64_t)B + PJ_BT - 1) / PJ_BT;
    p->groups = p->otiles * p->slices * p->bchunks;
    return p->groups <= NV_GRID_MAX;
}

// the projection's only workspace section: partial [slices][B][O]
struct NvWs {
    float* partial;
    size_t total;
};

NvWs nv_layout(void* base, int32_t B, int32_t O, int64_t slices)
{
    Carver c{base};
    NvWs w;
    w.partial = c.take<float>((size_t)slices * (size_t)B * (size_t)O);
    w.total = c.o;
    return w;
}

bool nv_bad_ptr(const void* p) { return !p || misaligned(p, 4); }

}  // namespace

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_netvlad_tiles(int32_t* n_step, int32_t* d_tile, int32_t* i_slice, int32_t* o_tile, int32_t* b_tile)
{
    if (!n_step || !d_tile || !i_slice || !o_tile || !b_tile) return SPLATRASTER_ERR_BAD_ARG;
    *n_step = NV_T;
    *d_tile = NV_DT;
    *i_slice = PJ_SLICE;
    *o_tile = PJ_OT;
    *b_tile = PJ_BT;
    return SPLATRASTER_OK;
}

int splatraster_netvlad_workspace_size(int32_t B, int32_t D, int32_t K, int32_t N, int32_t O, size_t* bytes)
{
    if (bytes) *bytes = 0;
    PjPlan p;
    if (!bytes || !nv_shape_ok(B, D, K, N) || !pj_shape_ok(B, O, (int64_t)D * K, &p)) return SPLATRASTER_ERR_BAD_ARG;
    *bytes = nv_layout(nullptr, B, O, p.slices).total;
    return SPLATRASTER_OK;
}

int splatraster_netvlad_assign(int32_t B, int32_t D, int32_t K, int32_t N, const float* features, const float* score_w,
                               const float* score_b, float* assign, float* inv_norm, void* workspace, size_t workspace_bytes,
                               void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    (void)workspace_bytes;   // the stage needs none of it
    if (!nv_shape_ok(B, D, K, N)) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (nv_bad_ptr(features) || nv_bad_ptr(score_w) || nv_bad_ptr(assign) || nv_bad_ptr(inv_norm)) return SPLATRASTER_ERR_BAD_ARG;
    if (misaligned(score_b, 4) || misaligned(workspace, 4)) return SPLATRASTER_ERR_BAD_ARG;
    const int32_t steps = (N + NV_T - 1) / NV_T;
    hipLaunchKernelGGL(netvlad_assign_kernel, dim3((unsigned)((int64_t)B * steps)), dim3(NV_ASSIGN_THREADS), 0, stream, D, K, N, steps,
                       features, score_w, score_b, assign, inv_norm);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_netvlad_aggregate(int32_t B, int32_t D, int32_t K, int32_t N, const float* features, const float* assign,
                                  const float* inv_norm, const float* centers, int32_t flags, float* v, void* workspace,
                                  size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    (void)workspace_bytes;   // the stage needs none of it
    if (!nv_shape_ok(B, D, K, N) || (flags & ~(SPLATRASTER_NETVLAD_INTRANORM | SPLATRASTER_NETVLAD_L2NORM))) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (nv_bad_ptr(features) || nv_bad_ptr(assign) || nv_bad_ptr(inv_norm) || nv_bad_ptr(centers) || nv_bad_ptr(v))
        return SPLATRASTER_ERR_BAD_ARG;
    if (misaligned(workspace, 4)) return SPLATRASTER_ERR_BAD_ARG;
    const int32_t dblocks = (D + NV_DT - 1) / NV_DT;
    hipLaunchKernelGGL(netvlad_aggregate_kernel, dim3((unsigned)((int64_t)B * dblocks)), dim3(NV_AGG_THREADS), 0, stream, D, K, N, dblocks,
                       features, assign, inv_norm, v);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(netvlad_finish_kernel, dim3((unsigned)B), dim3(NV_FIN_THREADS), 0, stream, D, K, N, assign, centers, flags, v);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_netvlad_project(int32_t B, int32_t O, int64_t I, const float* x, const float* weight, const float* bias, int32_t flags,
                                float* y, void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    PjPlan p;
    if (!pj_shape_ok(B, O, I, &p) || (flags & ~SPLATRASTER_NETVLAD_L2NORM)) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (nv_bad_ptr(x) || nv_bad_ptr(weight) || nv_bad_ptr(y) || misaligned(bias, 4) || nv_bad_ptr(workspace)) return SPLATRASTER_ERR_BAD_ARG;
    const NvWs w = nv_layout(workspace, B, O, p.slices);
    if (workspace_bytes < w.total) return SPLATRASTER_ERR_BAD_ARG;
    const bool vec = I % 4 == 0 && ((uintptr_t)x | (uintptr_t)weight) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL((netvlad_project_kernel<true>), dim3((unsigned)p.groups), dim3(PJ_THREADS), 0, stream, B, O, I, (int32_t)p.otiles,
                           (int32_t)p.slices, x, weight, w.partial);
    else
        hipLaunchKernelGGL((netvlad_project_kernel<false>), dim3((unsigned)p.groups), dim3(PJ_THREADS), 0, stream, B, O, I, (int32_t)p.otiles,
                           (int32_t)p.slices, x, weight, w.partial);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(netvlad_project_finish_kernel, dim3((unsigned)B), dim3(PJ_FIN_THREADS), 0, stream, B, O, (int32_t)p.slices,
                       (const float*)w.partial, bias, flags, y);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
