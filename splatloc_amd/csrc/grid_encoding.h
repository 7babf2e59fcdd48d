// grid_encoding.h — the device functions and the kernel-argument level table of the multiresolution grid encoding, shared by
// grid_encoding.hip (tinycudann.Encoding) and decoder.hip (the fused FeatureDecoder): both evaluate a (point, level) pair with
// exactly this arithmetic, so their encoded features are bit-identical.  Definition: include/splatraster.h
// (splatraster_grid_encoding_layout) and INTEGRATION.md §13.
#pragma once
#include "common.h"

#include <string.h>

namespace sr {

struct GridArgs {
    uint32_t offset[SPLATRASTER_GRID_MAX_LEVELS];
    uint32_t size[SPLATRASTER_GRID_MAX_LEVELS];
    uint32_t res[SPLATRASTER_GRID_MAX_LEVELS];
    float scale[SPLATRASTER_GRID_MAX_LEVELS];
    int32_t n_levels;
    int32_t lp_log2;   // lanes per point = 1 << lp_log2 >= n_levels
    int32_t hashed;    // grid type Hash: levels whose dense grid outgrows their size are hashed
};

template <int F>
struct Feat {
    float v[F];
};

template <int F>
__device__ __forceinline__ Feat<F> load_feat(const float* p)
{
    Feat<F> r;
    if constexpr (F == 1) {
        r.v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        r.v[0] = a.x; r.v[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 a = *reinterpret_cast<const float4*>(p + k);
            r.v[k] = a.x; r.v[k + 1] = a.y; r.v[k + 2] = a.z; r.v[k + 3] = a.w;
        }
    }
    return r;
}

template <int F>
__device__ __forceinline__ void store_feat(float* p, const float (&v)[F])
{
    if constexpr (F == 1) {
        p[0] = v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

// cell and fractional position of a point at one level (no clamping: outside [0, 1] wraps through uint32 arithmetic)
template <int D>
struct Locus {
    uint32_t cell[D];
    float frac[D];
};

template <int D>
__device__ __forceinline__ Locus<D> locate(float scale, const float* __restrict__ x)
{
    Locus<D> q;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float pos = fmaf(scale, x[d], 0.5f);
        const float fl = floorf(pos);
        q.cell[d] = (uint32_t)(int)fl;
        q.frac[d] = pos - fl;
    }
    return q;
}

// table index (within the level) of corner `c` (bit d set: cell_d + 1)
template <int D>
__device__ __forceinline__ uint32_t corner_index(const Locus<D>& q, int c, uint32_t res, uint32_t size, bool hashed)
{
    constexpr uint32_t PRIMES[3] = {1u, 2654435761u, 805459861u};
    uint32_t stride = 1, index = 0, hash = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const uint32_t g = q.cell[d] + ((c >> d) & 1);
        if (stride <= size) {          // dense index; stops growing once the stride passes the level's size
            index += g * stride;
            stride *= res;
        }
        hash ^= g * PRIMES[d];
    }
    if (hashed && size < stride) index = hash;
    return index % size;
}

// interpolation weight of corner c: product over dimensions of frac_d (bit set) or 1 - frac_d, in dimension order
template <int D>
__device__ __forceinline__ float corner_weight(const Locus<D>& q, int c)
{
    float w = 1.f;
#pragma unroll
    for (int d = 0; d < D; ++d) w *= ((c >> d) & 1) ? q.frac[d] : 1.f - q.frac[d];
    return w;
}

// a layout the kernels can index safely: the one splatraster_grid_encoding_layout() makes (offsets = running sum of sizes, sizes > 0)
static inline int grid_args(const splatraster_grid_layout* lay, GridArgs* a)
{
    if (!lay) return SPLATRASTER_ERR_BAD_ARG;
    const int D = lay->n_dims, L = lay->n_levels, F = lay->n_features;
    if ((D != 2 && D != 3) || (F != 1 && F != 2 && F != 4 && F != 8) || L < 1 || L > SPLATRASTER_GRID_MAX_LEVELS)
        return SPLATRASTER_ERR_UNSUPPORTED;
    uint64_t total = 0;
    for (int l = 0; l < L; ++l) {
        if (lay->size[l] == 0 || lay->offset[l] != total) return SPLATRASTER_ERR_BAD_ARG;
        total += lay->size[l];
    }
    if (total > 0x7fffffffull || lay->n_params != (int64_t)total * F) return SPLATRASTER_ERR_BAD_ARG;
    memcpy(a->offset, lay->offset, sizeof(a->offset));
    memcpy(a->size, lay->size, sizeof(a->size));
    memcpy(a->res, lay->resolution, sizeof(a->res));
    memcpy(a->scale, lay->scale, sizeof(a->scale));
    a->n_levels = L;
    int lp = 0;
    while ((1 << lp) < L) ++lp;
    a->lp_log2 = lp;
    a->hashed = lay->grid_type == SPLATRASTER_GRID_HASH;
    return SPLATRASTER_OK;
}

}  // namespace sr
