// grid_encoding.hip — tinycudann.Encoding (models/encoding.py:33-46): the multiresolution grid encoding of FeatureDecoder,
// forward and both gradients.  Definition: include/splatraster.h (splatraster_grid_encoding_layout) and INTEGRATION.md §13.
//
// gfx950 shape: one lane per (point, level), the level varying fastest.  A point owns Lp = next_pow2(L) consecutive lanes
// (lanes of levels >= L idle), so 64 / Lp points share a wave and the L lanes of a point never straddle two waves; at
// SplatLoc's L = 16, F = 2 a wave stores 4 whole 128-byte output rows, 512 contiguous bytes.  The level table (offset, size,
// resolution, scale) is computed once on the host and passed by value as the kernel argument, never recomputed per lane.
// Each lane computes its 2^D corner indices, issues every corner gather (one F*4-byte load per corner: 8 bytes at F = 2)
// before it uses any, and accumulates with fmaf in corner order.  The parameter gradient is one no-return
// global_atomic_add_f32 per (corner, feature); the input gradient is reduced over the Lp lanes of a point with xor shuffles
// and stored once per point.  No LDS, no scratch (tests/test_gpu_grid_encoding.py pins the latter).
#include "common.h"
#include "grid_encoding.h"

#include <math.h>
#include <string.h>

namespace sr {

constexpr int GRID_THREADS = 256;

template <int D, int F>
__global__ void __launch_bounds__(GRID_THREADS)
grid_encode_fwd_kernel(int64_t N, GridArgs a, const float* __restrict__ x, const float* __restrict__ params,
                       float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
    const int64_t n = t >> a.lp_log2;
    const int level = (int)(t & ((1 << a.lp_log2) - 1));
    if (n >= N || level >= a.n_levels) return;
    const Locus<D> q = locate<D>(a.scale[level], x + n * D);
    const uint32_t res = a.res[level], size = a.size[level];
    const float* grid = params + (size_t)a.offset[level] * F;
    constexpr int C = 1 << D;
    Feat<F> v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = load_feat<F>(grid + (size_t)corner_index<D>(q, c, res, size, a.hashed) * F);
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float w = corner_weight<D>(q, c);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = fmaf(w, v[c].v[f], acc[f]);
    }
    store_feat<F>(out + n * (int64_t)(a.n_levels * F) + level * F, acc);
}

template <int D, int F, bool PGRAD, bool XGRAD>
__global__ void __launch_bounds__(GRID_THREADS)
grid_encode_bwd_kernel(int64_t N, GridArgs a, const float* __restrict__ x, const float* __restrict__ params,
                       const float* __restrict__ dL_dout, float* __restrict__ dL_dparams, float* __restrict__ dL_dx)
{
    const int64_t t = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
    const int64_t n = t >> a.lp_log2;
    const int level = (int)(t & ((1 << a.lp_log2) - 1));
    const bool active = n < N && level < a.n_levels;
    if (!XGRAD && !active) return;        // with XGRAD every lane stays for the shuffles below
    float gx[D];
#pragma unroll
    for (int d = 0; d < D; ++d) gx[d] = 0.f;
    if (active) {
        const float scale = a.scale[level];
        const Locus<D> q = locate<D>(scale, x + n * D);
        const uint32_t res = a.res[level], size = a.size[level];
        const size_t base = (size_t)a.offset[level] * F;
        const Feat<F> g = load_feat<F>(dL_dout + n * (int64_t)(a.n_levels * F) + level * F);
        constexpr int C = 1 << D;
        uint32_t idx[C];
#pragma unroll
        for (int c = 0; c < C; ++c) idx[c] = corner_index<D>(q, c, res, size, a.hashed);
        Feat<F> v[C];
        if constexpr (XGRAD) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = load_feat<F>(params + base + (size_t)idx[c] * F);
        }
        if constexpr (PGRAD) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float w = corner_weight<D>(q, c);
                float* p = dL_dparams + base + (size_t)idx[c] * F;
#pragma unroll
                for (int f = 0; f < F; ++f) atomicAdd(p + f, w * g.v[f]);
            }
        }
        if constexpr (XGRAD) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float dot = 0.f;
#pragma unroll
                for (int f = 0; f < F; ++f) dot = fmaf(g.v[f], v[c].v[f], dot);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    // d/dpos_d of the corner weight: the other dimensions' factors, signed by the corner's side in d
                    float w = ((c >> d) & 1) ? scale : -scale;
#pragma unroll
                    for (int e = 0; e < D; ++e)
                        if (e != d) w *= ((c >> e) & 1) ? q.frac[e] : 1.f - q.frac[e];
                    gx[d] = fmaf(w, dot, gx[d]);
                }
            }
        }
    }
    if constexpr (XGRAD) {
        // sum over the Lp lanes of the point (aligned groups inside one wave)
        for (int m = (1 << a.lp_log2) >> 1; m >= 1; m >>= 1) {
#pragma unroll
            for (int d = 0; d < D; ++d) gx[d] += __shfl_xor(gx[d], m);
        }
        if (n < N && level == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) dL_dx[n * D + d] = gx[d];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static dim3 grid_blocks(int64_t N, const GridArgs& a)
{
    return dim3((unsigned)(((N << a.lp_log2) + GRID_THREADS - 1) / GRID_THREADS));
}

// lanes of all N points fit one 1-D grid (2^31 - 1 blocks): N <= 2^31 * 256 / 32 covers any table-sized batch
static bool grid_n_ok(int64_t N) { return N >= 0 && N <= (int64_t(1) << 36); }

template <int D, int F>
static void launch_fwd(int64_t N, const GridArgs& a, const float* x, const float* params, float* out, hipStream_t s)
{
    hipLaunchKernelGGL((grid_encode_fwd_kernel<D, F>), grid_blocks(N, a), dim3(GRID_THREADS), 0, s, N, a, x, params, out);
}

template <int D, int F>
static void launch_bwd(int64_t N, const GridArgs& a, const float* x, const float* params, const float* g, float* dp, float* dx,
                       hipStream_t s)
{
    const dim3 b = grid_blocks(N, a);
    if (dp && dx)
        hipLaunchKernelGGL((grid_encode_bwd_kernel<D, F, true, true>), b, dim3(GRID_THREADS), 0, s, N, a, x, params, g, dp, dx);
    else if (dp)
        hipLaunchKernelGGL((grid_encode_bwd_kernel<D, F, true, false>), b, dim3(GRID_THREADS), 0, s, N, a, x, params, g, dp, dx);
    else
        hipLaunchKernelGGL((grid_encode_bwd_kernel<D, F, false, true>), b, dim3(GRID_THREADS), 0, s, N, a, x, params, g, dp, dx);
}

#define SR_GRID_DISPATCH(D, F, CALL)                           \
    do {                                                       \
        switch ((D) * 16 + (F)) {                              \
        case 2 * 16 + 1: CALL(2, 1); break;                    \
        case 2 * 16 + 2: CALL(2, 2); break;                    \
        case 2 * 16 + 4: CALL(2, 4); break;                    \
        case 2 * 16 + 8: CALL(2, 8); break;                    \
        case 3 * 16 + 1: CALL(3, 1); break;                    \
        case 3 * 16 + 2: CALL(3, 2); break;                    \
        case 3 * 16 + 4: CALL(3, 4); break;                    \
        case 3 * 16 + 8: CALL(3, 8); break;                    \
        default: return SPLATRASTER_ERR_UNSUPPORTED;           \
        }                                                      \
    } while (0)

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_grid_encoding_layout(int32_t D, int32_t L, int32_t F, int32_t log2_T, int32_t base_res, double per_level_scale,
                                     int32_t grid_type, splatraster_grid_layout* out)
{
#pragma clang fp contract(off)   // the level table rounds each f32 operation on its own (no fused multiply-add)
    if (!out) return SPLATRASTER_ERR_BAD_ARG;
    if (D != 2 && D != 3) return SPLATRASTER_ERR_UNSUPPORTED;
    if (F != 1 && F != 2 && F != 4 && F != 8) return SPLATRASTER_ERR_UNSUPPORTED;
    if (L < 1 || L > SPLATRASTER_GRID_MAX_LEVELS) return SPLATRASTER_ERR_UNSUPPORTED;
    if (grid_type != SPLATRASTER_GRID_HASH && grid_type != SPLATRASTER_GRID_DENSE && grid_type != SPLATRASTER_GRID_TILED)
        return SPLATRASTER_ERR_UNSUPPORTED;
    if (grid_type == SPLATRASTER_GRID_HASH && (log2_T < 1 || log2_T > 30)) return SPLATRASTER_ERR_UNSUPPORTED;
    if (base_res < 1 || !(per_level_scale > 0.0) || !isfinite(per_level_scale)) return SPLATRASTER_ERR_BAD_ARG;
    splatraster_grid_layout r;
    memset(&r, 0, sizeof(r));
    r.n_dims = D;
    r.n_levels = L;
    r.n_features = F;
    r.grid_type = grid_type;
    const float log2_b = log2f((float)per_level_scale);
    const uint64_t max_dense = 0x7fffffffull;     // a level's dense entry count saturates here (before rounding up to 8)
    uint64_t total = 0;
    for (int l = 0; l < L; ++l) {
        const float scale = exp2f((float)l * log2_b) * (float)base_res - 1.0f;
        if (!isfinite(scale) || scale < 0.f || scale >= 2147483648.0f) return SPLATRASTER_ERR_UNSUPPORTED;
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        uint64_t dense = 1;
        for (int d = 0; d < D && dense <= max_dense; ++d) dense *= res;
        if (dense > max_dense) dense = max_dense;
        uint64_t size = (dense + 7) / 8 * 8;
        if (grid_type == SPLATRASTER_GRID_HASH) {
            size = size < (1ull << log2_T) ? size : (1ull << log2_T);
        } else if (grid_type == SPLATRASTER_GRID_TILED) {
            uint64_t tile = 1;
            for (int d = 0; d < D; ++d) tile *= (uint64_t)base_res;
            size = size < tile ? size : tile;
        }
        r.offset[l] = (uint32_t)total;
        r.size[l] = (uint32_t)size;
        r.resolution[l] = res;
        r.scale[l] = scale;
        total += size;
        if (total > max_dense) return SPLATRASTER_ERR_UNSUPPORTED;   // entry indices stay below 2^31
    }
    r.n_params = (int64_t)total * F;
    *out = r;
    return SPLATRASTER_OK;
}

int splatraster_grid_encoding_forward(const splatraster_grid_layout* lay, int64_t N, const float* x, const float* params, float* out,
                                      void* stream)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GridArgs a;
    const int st = grid_args(lay, &a);
    if (st) return st;
    if (!grid_n_ok(N)) return SPLATRASTER_ERR_BAD_ARG;
    if (N == 0) return SPLATRASTER_OK;
    if (!x || !params || !out || (reinterpret_cast<uintptr_t>(params) & 15u) || (reinterpret_cast<uintptr_t>(out) & 15u))
        return SPLATRASTER_ERR_BAD_ARG;
#define SR_CALL(d, f) launch_fwd<d, f>(N, a, x, params, out, s)
    SR_GRID_DISPATCH(lay->n_dims, lay->n_features, SR_CALL);
#undef SR_CALL
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_grid_encoding_backward(const splatraster_grid_layout* lay, int64_t N, const float* x, const float* params,
                                       const float* dL_dout, float* dL_dparams, float* dL_dx, void* stream)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GridArgs a;
    const int st = grid_args(lay, &a);
    if (st) return st;
    if (!grid_n_ok(N)) return SPLATRASTER_ERR_BAD_ARG;
    if (N == 0 || (!dL_dparams && !dL_dx)) return SPLATRASTER_OK;
    if (!x || !dL_dout || (dL_dx && !params)) return SPLATRASTER_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(dL_dout) & 15u) || (dL_dx && (reinterpret_cast<uintptr_t>(params) & 15u)) ||
        (reinterpret_cast<uintptr_t>(dL_dparams) & 15u))
        return SPLATRASTER_ERR_BAD_ARG;
#define SR_CALL(d, f) launch_bwd<d, f>(N, a, x, params, dL_dout, dL_dparams, dL_dx, s)
    SR_GRID_DISPATCH(lay->n_dims, lay->n_features, SR_CALL);
#undef SR_CALL
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
