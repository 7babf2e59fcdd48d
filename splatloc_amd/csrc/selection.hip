// selection.hip — SplatLoc's landmark selection (utils/selection.py:91-157, gaussian_selectition): the per-point saliency
// score over the training views and the greedy spatial pick.  Definition: include/splatraster.h (splatraster_landmark_*)
// and INTEGRATION.md §16.
//
// gfx950 shape.  Scores: one lane per point, 256 lanes per block; the views' [R|t] are staged in LDS as f64 in chunks of
// SEL_VIEW_CHUNK and every lane walks them in order (all lanes read the same LDS word: broadcast).  The depth gather is one
// scattered 4-byte load per visible (point, view) pair from the single [M, H, W] stack, offsets in 64 bits.  The 3x3
// eigenproblem is a cyclic Jacobi in f64 with a fixed sweep bound.
//
// Pick: the scores are sorted by two stable LSD passes of sort_pairs_u32 over an order-preserving 64-bit key (ties: the
// larger index first).  Then, per pass of the reference's loop at radius r:
//   filter   every candidate in parallel against the landmarks of earlier passes (LDS-staged, 256 at a time);
//   compact  the survivors in priority order (exclusive_scan_u32 + scatter);
//   resolve  one workgroup walks the survivors in chunks of 1024: each checks against the landmarks taken earlier in this
//            pass, then the chunk is resolved in priority order by ballots (each round takes the first live candidate and
//            kills the live ones within r of it; one barrier per round).
// A candidate's fate depends only on the candidates ahead of it, so this is the reference's pick exactly.  The host reads
// the landmark count back once per pass.  The whole file is compiled without FP contraction (build.py NO_CONTRACT): the
// distance sqrt((dx*dx + dy*dy) + dz*dz) < r must round like numpy's norm.
#include "common.h"

#include <math.h>

namespace sr {

constexpr int SEL_THREADS = 256;
constexpr int SEL_VIEW_CHUNK = 64;
constexpr int SEL_RESOLVE_THREADS = 1024;
constexpr int SEL_RESOLVE_WAVES = SEL_RESOLVE_THREADS / WAVE;
// landmarks of the current pass kept in LDS by the resolve kernel: 4096 float4 = 64 KB.  With the 1024 candidates (16 KB)
// and the ballot masks (256 B) sel_resolve_kernel holds 82 176 B of static LDS; later landmarks are read from global memory
constexpr int SEL_LDS_LANDMARKS = 4096;
constexpr int SEL_JACOBI_SWEEPS = 16;      // cyclic Jacobi on 3x3 converges in <= 6 sweeps in f64; hard bound
constexpr int SEL_MAX_PASSES = 1100;       // 18 * 2^-1100 == 0 in f64: the radius has underflowed long before

struct SelK {
    double k[9];
};

// eigenvalues of the symmetric 3x3 [a00 a01 a02; . a11 a12; . . a22]: min and max
__device__ __forceinline__ void sym3_eig_minmax(double a00, double a01, double a02, double a11, double a12, double a22,
                                                double* lmin, double* lmax)
{
    for (int sweep = 0; sweep < SEL_JACOBI_SWEEPS; ++sweep) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        if (off == 0.0) break;
        // rotation (p, q) zeroing a_pq, for (0,1), (0,2), (1,2)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double app, aqq, apq, apk, aqk;   // k: the third index
            if (r == 0) { app = a00; aqq = a11; apq = a01; apk = a02; aqk = a12; }
            else if (r == 1) { app = a00; aqq = a22; apq = a02; apk = a01; aqk = a12; }
            else { app = a11; aqq = a22; apq = a12; apk = a01; aqk = a02; }
            if (apq == 0.0) continue;
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0);
            const double s = t * c;
            const double npp = app - t * apq;
            const double nqq = aqq + t * apq;
            const double npk = c * apk - s * aqk;
            const double nqk = s * apk + c * aqk;
            if (r == 0) { a00 = npp; a11 = nqq; a01 = 0.0; a02 = npk; a12 = nqk; }
            else if (r == 1) { a00 = npp; a22 = nqq; a02 = 0.0; a01 = npk; a12 = nqk; }
            else { a11 = npp; a22 = nqq; a12 = 0.0; a01 = npk; a02 = nqk; }
        }
    }
    *lmin = fmin(a00, fmin(a11, a22));
    *lmax = fmax(a00, fmax(a11, a22));
}

// python's min(2, x): x when x < 2 (false for NaN), else 2
__device__ __forceinline__ double py_min2(double x) { return x < 2.0 ? x : 2.0; }

__global__ void __launch_bounds__(SEL_THREADS)
landmark_scores_kernel(int64_t N, int32_t M, const float* __restrict__ points, const float* __restrict__ w2c, SelK K,
                       const float* __restrict__ depths, int32_t W, int32_t H, int32_t* __restrict__ n_visible,
                       int32_t* __restrict__ n_depth, double* __restrict__ depth_mean, double* __restrict__ depth_std,
                       double* __restrict__ span, double* __restrict__ score)
{
    __shared__ double s_view[SEL_VIEW_CHUNK][12];   // R row-major, then t
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool live = i < N;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (live) {
        px = (double)points[i * 3 + 0];
        py = (double)points[i * 3 + 1];
        pz = (double)points[i * 3 + 2];
    }
    const double Wd = (double)W, Hd = (double)H;
    const int64_t plane = (int64_t)W * H;
    int nvis = 0, nd = 0;
    double x0 = 0.0, s1 = 0.0, s2 = 0.0;                          // kept diffs, shifted by the first one
    double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
    for (int v0 = 0; v0 < M; v0 += SEL_VIEW_CHUNK) {
        const int nv = min(SEL_VIEW_CHUNK, M - v0);
        __syncthreads();
        for (int e = threadIdx.x; e < nv * 12; e += SEL_THREADS) {
            const int v = e / 12, k = e % 12;
            const int src = k < 9 ? (k / 3) * 4 + (k % 3) : (k - 9) * 4 + 3;
            s_view[v][k] = (double)w2c[(int64_t)(v0 + v) * 16 + src];
        }
        __syncthreads();
        if (!live) continue;
        for (int v = 0; v < nv; ++v) {
            const double* m = s_view[v];
            const double cx = m[0] * px + m[1] * py + m[2] * pz + m[9];
            const double cy = m[3] * px + m[4] * py + m[5] * pz + m[10];
            const double cz = m[6] * px + m[7] * py + m[8] * pz + m[11];
            if (cz < 0.01) continue;
            const double q0 = K.k[0] * cx + K.k[1] * cy + K.k[2] * cz;
            const double q1 = K.k[3] * cx + K.k[4] * cy + K.k[5] * cz;
            const double q2 = K.k[6] * cx + K.k[7] * cy + K.k[8] * cz;
            const double u = q0 / q2, w = q1 / q2;
            if (!(u < Wd && u > 0.0 && w < Hd && w > 0.0)) continue;
            ++nvis;
            const float d = depths[(int64_t)(v0 + v) * plane + (int64_t)(int)w * W + (int)u];
            const double dd = (double)d;
            const double diff = fabs(cz - dd);
            if (diff < 0.3 && dd > 0.02) {
                if (nd == 0) x0 = diff;
                const double y = diff - x0;
                s1 += y;
                s2 += y * y;
                ++nd;
            }
            // the reference's b = R^T (p - t), normalised; H += I - b b^T
            const double ex = px - m[9], ey = py - m[10], ez = pz - m[11];
            double bx = m[0] * ex + m[3] * ey + m[6] * ez;
            double by = m[1] * ex + m[4] * ey + m[7] * ez;
            double bz = m[2] * ex + m[5] * ey + m[8] * ez;
            const double nb = sqrt(bx * bx + by * by + bz * bz);
            bx /= nb; by /= nb; bz /= nb;
            h00 += 1.0 - bx * bx; h01 -= bx * by; h02 -= bx * bz;
            h11 += 1.0 - by * by; h12 -= by * bz;
            h22 += 1.0 - bz * bz;
        }
    }
    if (!live) return;
    double mean = __builtin_nan(""), sd = __builtin_nan("");
    if (nd > 0) {
        const double a = s1 / nd;
        mean = x0 + a;
        const double var = s2 / nd - a * a;
        sd = sqrt(var > 0.0 ? var : 0.0);
    }
    double sp = 0.0;
    if (nvis > 0) {
        const double inv = (double)nvis;
        double lmin, lmax;
        sym3_eig_minmax(h00 / inv, h01 / inv, h02 / inv, h11 / inv, h12 / inv, h22 / inv, &lmin, &lmax);
        double c = 1.0 - 2.0 * lmin / lmax;
        // numpy's clip(c, 0, 1) keeps NaN
        c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
        sp = acos(c);
    }
    // min(2, 0.05 / mean) + min(2, 0.05 / std): NaN (no diff kept) -> 2, 0 -> inf -> 2
    const double ds = py_min2(0.05 / mean) + py_min2(0.05 / sd);
    n_visible[i] = nvis;
    n_depth[i] = nd;
    depth_mean[i] = mean;
    depth_std[i] = sd;
    span[i] = sp;
    score[i] = ds + sp;
}

// ---- sort: ascending stable by an order-preserving key of the score, read back to front ------------------------------------
__device__ __forceinline__ uint64_t score_key(double s)
{
    uint64_t b = (s != s) ? 0x7ff8000000000000ull : (s == 0.0 ? 0ull : (uint64_t)__double_as_longlong(s));   // NaN last
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(SEL_THREADS)
sel_key_lo_kernel(int64_t N, const double* __restrict__ score, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i >= N) return;
    keys[i] = (uint32_t)score_key(score[i]);
    vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(SEL_THREADS)
sel_key_hi_kernel(int64_t N, const double* __restrict__ score, const uint32_t* __restrict__ perm, uint32_t* __restrict__ keys)
{
    const int64_t j = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (j >= N) return;
    keys[j] = (uint32_t)(score_key(score[perm[j]]) >> 32);
}

// rank j (0 = highest priority) -> original index and position; the first landmark is rank 0
__global__ void __launch_bounds__(SEL_THREADS)
sel_rank_kernel(int64_t N, const uint32_t* __restrict__ perm, const float* __restrict__ points, int32_t* __restrict__ order,
                float4* __restrict__ pos, float4* __restrict__ landmarks, int32_t* __restrict__ out_idx,
                uint32_t* __restrict__ count)
{
    const int64_t j = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (j >= N) return;
    const uint32_t idx = perm[N - 1 - j];
    order[j] = (int32_t)idx;
    const float4 p = make_float4(points[(int64_t)idx * 3], points[(int64_t)idx * 3 + 1], points[(int64_t)idx * 3 + 2], 0.f);
    pos[j] = p;
    if (j == 0) {
        landmarks[0] = p;
        out_idx[0] = (int32_t)idx;
        *count = 1u;
    }
}

// numpy: norm(xyz.reshape(3, 1) - selected, axis=0) < radius, in f64 (the f32 point widened), no contraction
__device__ __forceinline__ bool sel_near(float4 a, float4 b, double radius)
{
    const double dx = (double)a.x - (double)b.x;
    const double dy = (double)a.y - (double)b.y;
    const double dz = (double)a.z - (double)b.z;
    return sqrt((dx * dx + dy * dy) + dz * dz) < radius;
}

// flags[j] = 1 iff candidate j is farther than radius from every landmark taken before this pass
__global__ void __launch_bounds__(SEL_THREADS)
sel_filter_kernel(int64_t N, const float4* __restrict__ pos, const float4* __restrict__ landmarks,
                  const uint32_t* __restrict__ count, double radius, uint32_t* __restrict__ flags)
{
    __shared__ float4 s_l[SEL_THREADS];
    const int64_t j = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t L = *count;
    const float4 p = j < N ? pos[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    int alive = j < N;
    for (uint32_t l0 = 0; l0 < L; l0 += SEL_THREADS) {
        const uint32_t nl = min((uint32_t)SEL_THREADS, L - l0);
        __syncthreads();
        if (threadIdx.x < nl) s_l[threadIdx.x] = landmarks[l0 + threadIdx.x];
        __syncthreads();
        if (alive)
            for (uint32_t l = 0; l < nl; ++l)
                if (sel_near(p, s_l[l], radius)) { alive = 0; break; }
        if (!__syncthreads_or(alive)) break;
    }
    if (j < N) flags[j] = (uint32_t)alive;
}

// offsets (exclusive scan of the flags) -> survivors in priority order
__global__ void __launch_bounds__(SEL_THREADS)
sel_scatter_kernel(int64_t N, const uint32_t* __restrict__ offs, const uint64_t* __restrict__ total,
                   uint32_t* __restrict__ surv)
{
    const int64_t j = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (j >= N) return;
    const uint32_t next = j + 1 < N ? offs[j + 1] : (uint32_t)*total;
    if (next != offs[j]) surv[offs[j]] = (uint32_t)j;
}

// one workgroup: the survivors in priority order, the reference's sequential decision per candidate
__global__ void __launch_bounds__(SEL_RESOLVE_THREADS)
sel_resolve_kernel(const uint32_t* __restrict__ surv, const uint64_t* __restrict__ total, const float4* __restrict__ pos,
                   const int32_t* __restrict__ order, double radius, uint32_t num, float4* __restrict__ landmarks,
                   int32_t* __restrict__ out_idx, uint32_t* __restrict__ count)
{
    __shared__ float4 s_new[SEL_LDS_LANDMARKS];
    __shared__ float4 s_cand[SEL_RESOLVE_THREADS];
    __shared__ uint64_t s_mask[2][SEL_RESOLVE_WAVES];
    const uint32_t S = (uint32_t)*total;
    const uint32_t L0 = *count;
    uint32_t L = L0;
    const int t = threadIdx.x, wave = t / WAVE, lane = t % WAVE;
    int parity = 0;
    for (uint32_t c0 = 0; c0 < S && L < num; c0 += SEL_RESOLVE_THREADS) {
        const uint32_t k = c0 + t;
        uint32_t rank = 0;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        int alive = k < S;
        if (alive) {
            rank = surv[k];
            p = pos[rank];
        }
        s_cand[t] = p;
        // against the landmarks taken earlier in this pass
        if (alive) {
            const uint32_t nl = L - L0;
            for (uint32_t l = 0; l < nl; ++l) {
                const float4 q = l < SEL_LDS_LANDMARKS ? s_new[l] : landmarks[L0 + l];
                if (sel_near(p, q, radius)) { alive = 0; break; }
            }
        }
        // in-chunk resolution: every round takes the first live candidate (<= 1024 rounds, each kills at least one)
        for (int round = 0; round < SEL_RESOLVE_THREADS; ++round) {
            const uint64_t m = __ballot(alive);
            if (lane == 0) s_mask[parity][wave] = m;
            __syncthreads();
            int first = -1;
            for (int w = 0; w < SEL_RESOLVE_WAVES; ++w) {
                const uint64_t mw = s_mask[parity][w];
                if (mw) { first = w * WAVE + __ffsll((unsigned long long)mw) - 1; break; }
            }
            parity ^= 1;
            if (first < 0) break;
            const float4 q = s_cand[first];
            if (t == first) {
                landmarks[L] = q;
                out_idx[L] = order[rank];
                alive = 0;
            }
            if (L - L0 < SEL_LDS_LANDMARKS && t == 0) s_new[L - L0] = q;
            ++L;
            if (L >= num) break;
            if (alive && sel_near(p, q, radius)) alive = 0;
        }
        __syncthreads();   // s_cand / s_new of this chunk before the next one
    }
    if (t == 0) *count = L;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline unsigned sel_blocks(int64_t n) { return (unsigned)((n + SEL_THREADS - 1) / SEL_THREADS); }

struct SelWs {
    uint32_t *keys, *vals, *keys_alt, *vals_alt, *flags, *surv, *count;
    uint64_t* total;
    int32_t* order;
    float4 *pos, *landmarks;
    void *sort_tmp, *scan_tmp;
    size_t bytes;
};

static SelWs sel_layout(void* base, int64_t N, int32_t num)
{
    SelWs w;
    Carver c{base};
    const size_t n = (size_t)(N > 0 ? N : 1);
    w.keys = c.take<uint32_t>(n);
    w.vals = c.take<uint32_t>(n);
    w.keys_alt = c.take<uint32_t>(n);
    w.vals_alt = c.take<uint32_t>(n);
    w.flags = c.take<uint32_t>(n);
    w.surv = c.take<uint32_t>(n);
    w.order = c.take<int32_t>(n);
    w.pos = c.take<float4>(n);
    w.landmarks = c.take<float4>((size_t)(num > 0 ? num : 1));
    w.count = c.take<uint32_t>(1);
    w.total = c.take<uint64_t>(1);
    w.sort_tmp = c.take<char>(sort_tmp_bytes(N));
    w.scan_tmp = c.take<char>(scan_tmp_bytes(N));
    w.bytes = c.o;
    return w;
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_landmark_scores(int64_t N, int32_t M, const float* points, const float* w2c, const double* K,
                                const float* depths, int32_t width, int32_t height, int32_t* n_visible, int32_t* n_depth,
                                double* depth_mean, double* depth_std, double* span, double* score, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (N < 0 || M < 0 || width <= 0 || height <= 0 || !K) return SPLATRASTER_ERR_BAD_ARG;
    if (N == 0) return SPLATRASTER_OK;
    if (!points || !n_visible || !n_depth || !depth_mean || !depth_std || !span || !score) return SPLATRASTER_ERR_BAD_ARG;
    if (M > 0 && (!w2c || !depths)) return SPLATRASTER_ERR_BAD_ARG;
    if (N > ((int64_t)1 << 31) * SEL_THREADS) return SPLATRASTER_ERR_OVERFLOW;
    SelK k;
    for (int e = 0; e < 9; ++e) k.k[e] = K[e];
    hipLaunchKernelGGL(landmark_scores_kernel, dim3(sel_blocks(N)), dim3(SEL_THREADS), 0, stream, N, M, points, w2c, k,
                       depths, width, height, n_visible, n_depth, depth_mean, depth_std, span, score);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

size_t splatraster_landmark_workspace_bytes(int64_t N, int32_t num) { return sel_layout(nullptr, N, num).bytes; }

int splatraster_landmark_select(int64_t N, const float* points, const double* score, int32_t num, double radius,
                                int32_t* out_idx, int32_t* n_passes, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (n_passes) *n_passes = 0;
    if (N < 1 || num < 1 || num > N || !points || !score || !out_idx || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (!(radius > 0.0) || radius != radius || radius > 1e300) return SPLATRASTER_ERR_BAD_ARG;
    if (N >= ((int64_t)1 << 31)) return SPLATRASTER_ERR_OVERFLOW;
    const SelWs w = sel_layout(workspace, N, num);
    const unsigned nb = sel_blocks(N);
    bool alt = false;
    hipLaunchKernelGGL(sel_key_lo_kernel, dim3(nb), dim3(SEL_THREADS), 0, stream, N, score, w.keys, w.vals);
    SR_LAUNCH_CHECK();
    int st = sort_pairs_u32(N, w.keys, w.vals, w.keys_alt, w.vals_alt, 32, w.sort_tmp, stream, &alt, false);
    if (st != SPLATRASTER_OK) return st;
    uint32_t* perm = alt ? w.vals_alt : w.vals;
    uint32_t* kbuf = alt ? w.keys_alt : w.keys;
    uint32_t* perm_alt = alt ? w.vals : w.vals_alt;
    uint32_t* kbuf_alt = alt ? w.keys : w.keys_alt;
    hipLaunchKernelGGL(sel_key_hi_kernel, dim3(nb), dim3(SEL_THREADS), 0, stream, N, score, perm, kbuf);
    SR_LAUNCH_CHECK();
    st = sort_pairs_u32(N, kbuf, perm, kbuf_alt, perm_alt, 32, w.sort_tmp, stream, &alt, false);
    if (st != SPLATRASTER_OK) return st;
    if (alt) perm = perm_alt;
    hipLaunchKernelGGL(sel_rank_kernel, dim3(nb), dim3(SEL_THREADS), 0, stream, N, perm, points, w.order, w.pos, w.landmarks,
                       out_idx, w.count);
    SR_LAUNCH_CHECK();
    uint32_t taken = 1;
    int passes = 0;
    // the reference's while loop: one pass per radius, halved after each full pass; one host read per pass
    while (taken < (uint32_t)num) {
        if (passes >= SEL_MAX_PASSES || !(radius > 0.0)) {
            set_error_text("landmark_select: the radius underflowed before num landmarks were taken "
                           "(fewer than num distinct positions)");
            return SPLATRASTER_ERR_BAD_ARG;
        }
        hipLaunchKernelGGL(sel_filter_kernel, dim3(nb), dim3(SEL_THREADS), 0, stream, N, w.pos, w.landmarks, w.count, radius,
                           w.flags);
        SR_LAUNCH_CHECK();
        st = exclusive_scan_u32(N, w.flags, reinterpret_cast<uint32_t*>(w.total), w.scan_tmp, stream, false);
        if (st != SPLATRASTER_OK) return st;
        hipLaunchKernelGGL(sel_scatter_kernel, dim3(nb), dim3(SEL_THREADS), 0, stream, N, w.flags, w.total, w.surv);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sel_resolve_kernel, dim3(1), dim3(SEL_RESOLVE_THREADS), 0, stream, w.surv, w.total, w.pos, w.order,
                           radius, (uint32_t)num, w.landmarks, out_idx, w.count);
        SR_LAUNCH_CHECK();
        SR_HIP_CHECK(hipMemcpyAsync(&taken, w.count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SR_HIP_CHECK(hipStreamSynchronize(stream));
        ++passes;
        radius *= 0.5;
    }
    if (n_passes) *n_passes = passes;
    return SPLATRASTER_OK;
}

}  // extern "C"
