// fusion.hip — SplatLoc's feature-TSDF fusion (utils/fusion_utils.py: integrate, lines 112-181, and the vertex / feature gather of
// get_mesh, lines 277-288) on the device.  Definition: include/splatraster.h (splatraster_fusion_*) and INTEGRATION.md §20.
//
// gfx950 shape.  Integration: one lane per voxel in linear [X, Y, Z] order (consecutive lanes run along z), 256 lanes per block.
// Phase 1 walks the F <= 8 frames of the batch in order and keeps tsdf, weight and colour in registers; every frame in which the
// voxel is valid sets one bit of a per-lane mask.  Phase 2 ballots the lanes with a non-empty mask and walks the set bits: the
// whole wave takes one voxel's feature row (lane l owns channels 4l .. 4l+3: C = 256 is one global_load_dwordx4 and one
// global_store_dwordx4 per row), replays that voxel's valid frames in order with the row in registers, and writes it once.  A
// voxel's pixel in a frame is recomputed from its centre (broadcast with readlane) by the same function phase 1 used, so no
// per-frame state is kept and nothing is indexed dynamically in registers.  All element offsets are 64-bit.  The arithmetic is
// the reference's, one rounding per operation (build.py NO_CONTRACT): a batch is the same sequence of operations as F single
// launches, hence bit-identical to them.
//
// Surface: min / max reduction -> level, a count pass over the +x, +y, +z edges of every voxel, exclusive_scan_u32, a write pass
// in (voxel, axis) order, and a row gather (one wave per vertex).  Everything is order-independent or ordered: two runs agree
// bit for bit.
#include "fusion.h"

#include <math.h>

namespace sr {

struct FusFrames {
    float w2c[FUS_MAX_FRAMES][12];   // rows 0..2 of world-to-camera, row-major
    float intr[FUS_MAX_FRAMES][4];   // fx, fy, cx, cy
};

__device__ __forceinline__ float lane_f32(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// torch.clamp(v, 0, 255): NaN stays NaN
__device__ __forceinline__ float clamp_0_255(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }

// pixel of the voxel centre (wx, wy, wz) in frame f: fusion_utils.py:131-141.  cam = ((m0 x + m1 y) + m2 z) + m3 with separate
// roundings, pix = rint((cam * f) / z + c) (half to even, as torch.round); z > 0 is tested before anything becomes an integer
__device__ __forceinline__ bool fus_project(const FusFrames& fr, int f, float wx, float wy, float wz, int W, int H, int* pix,
                                            float* z)
{
    const float* m = fr.w2c[f];
    const float cx = ((m[0] * wx + m[1] * wy) + m[2] * wz) + m[3];
    const float cy = ((m[4] * wx + m[5] * wy) + m[6] * wz) + m[7];
    const float cz = ((m[8] * wx + m[9] * wy) + m[10] * wz) + m[11];
    if (!(cz > 0.f)) return false;
    const float px = rintf((cx * fr.intr[f][0]) / cz + fr.intr[f][2]);
    const float py = rintf((cy * fr.intr[f][1]) / cz + fr.intr[f][3]);
    if (!(px >= 0.f && px < (float)W && py >= 0.f && py < (float)H)) return false;
    *pix = (int)py * W + (int)px;
    *z = cz;
    return true;
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_integrate_kernel(int64_t N, int32_t Y, int32_t Z, int32_t C, const float* __restrict__ ax, const float* __restrict__ ay,
                        const float* __restrict__ az, float* __restrict__ tsdf, float* __restrict__ weight,
                        float* __restrict__ color, float* __restrict__ feat, int32_t F, int32_t H, int32_t W,
                        const float* __restrict__ depth, const float* __restrict__ color_im, const float* __restrict__ feat_im,
                        FusFrames fr, float obs, float trunc)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t n = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    const bool live = n < N;
    const int64_t HW = (int64_t)H * W;
    float wx = 0.f, wy = 0.f, wz = 0.f, w0 = 0.f;
    uint32_t mask = 0;
    if (live) {
        const int64_t YZ = (int64_t)Y * Z;
        const int32_t x = (int32_t)(n / YZ);
        const int32_t r = (int32_t)(n - (int64_t)x * YZ);
        const int32_t y = r / Z;
        wx = ax[x];
        wy = ay[y];
        wz = az[r - y * Z];
        w0 = weight[n];
        float w = w0, t = tsdf[n];
        float c0 = color[n * 3 + 0], c1 = color[n * 3 + 1], c2 = color[n * 3 + 2];
        for (int f = 0; f < F; ++f) {
            int pix;
            float cz;
            if (!fus_project(fr, f, wx, wy, wz, W, H, &pix, &cz)) continue;
            const int64_t p = (int64_t)f * HW + pix;
            const float d = depth[p];
            const float diff = d - cz;
            if (!(d > 0.f && diff >= -trunc)) continue;
            const float q = diff / trunc;
            const float dist = q > 1.f ? 1.f : q;
            const float wn = w + obs;
            t = (w * t + obs * dist) / wn;
            c0 = clamp_0_255(rintf((w * c0 + obs * color_im[p * 3 + 0]) / wn));
            c1 = clamp_0_255(rintf((w * c1 + obs * color_im[p * 3 + 1]) / wn));
            c2 = clamp_0_255(rintf((w * c2 + obs * color_im[p * 3 + 2]) / wn));
            w = wn;
            mask |= 1u << f;
        }
        if (mask) {
            tsdf[n] = t;
            weight[n] = w;
            color[n * 3 + 0] = c0;
            color[n * 3 + 1] = c1;
            color[n * 3 + 2] = c2;
        }
    }
    // feature rows: the wave takes the valid voxels one at a time
    const int64_t wave_base = n - lane;
    const bool owns = lane * 4 < C;
    uint64_t todo = __ballot(mask != 0);
    while (todo) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
        todo &= todo - 1;
        uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)mask, src);
        const float sx = lane_f32(wx, src), sy = lane_f32(wy, src), sz = lane_f32(wz, src);
        float w = lane_f32(w0, src);
        float4* row_ptr = reinterpret_cast<float4*>(feat + (wave_base + src) * C) + lane;
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        if (owns) row = *row_ptr;
        while (m) {
            const int f = __ffs(m) - 1;
            m &= m - 1;
            int pix = 0;
            float cz;
            fus_project(fr, f, sx, sy, sz, W, H, &pix, &cz);
            const float wn = w + obs;
            if (owns) {
                const float4 im = reinterpret_cast<const float4*>(feat_im + ((int64_t)f * HW + pix) * C)[lane];
                row.x = clamp_0_255((w * row.x + obs * im.x) / wn);
                row.y = clamp_0_255((w * row.y + obs * im.y) / wn);
                row.z = clamp_0_255((w * row.z + obs * im.z) / wn);
                row.w = clamp_0_255((w * row.w + obs * im.w) / wn);
            }
            w = wn;
        }
        if (owns) *row_ptr = row;
    }
}

// ---- surface -------------------------------------------------------------------------------------------------------------
// min and max of the block's values (NaN ignored, as fminf / fmaxf do), valid in thread 0
__device__ __forceinline__ void fus_block_minmax(float& lo, float& hi)
{
    __shared__ float s_lo[FUS_THREADS / WAVE], s_hi[FUS_THREADS / WAVE];
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_down(lo, o));
        hi = fmaxf(hi, __shfl_down(hi, o));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        s_lo[threadIdx.x / WAVE] = lo;
        s_hi[threadIdx.x / WAVE] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < FUS_THREADS / WAVE; ++k) {
            lo = fminf(lo, s_lo[k]);
            hi = fmaxf(hi, s_hi[k]);
        }
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_minmax_kernel(int64_t N, const float* __restrict__ tsdf, float* __restrict__ partial)
{
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * FUS_THREADS) {
        const float t = tsdf[i];
        lo = fminf(lo, t);
        hi = fmaxf(hi, t);
    }
    fus_block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = lo;
        partial[2 * blockIdx.x + 1] = hi;
    }
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_level_kernel(int32_t G, const float* __restrict__ partial, float* __restrict__ level)
{
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < G; i += FUS_THREADS) {
        lo = fminf(lo, partial[2 * i]);
        hi = fmaxf(hi, partial[2 * i + 1]);
    }
    fus_block_minmax(lo, hi);
    if (threadIdx.x == 0) *level = 0.5f * (lo + hi);
}

__global__ void fusion_set_level_kernel(float value, float* __restrict__ level) { *level = value; }

__global__ void __launch_bounds__(FUS_THREADS)
fusion_count_kernel(int64_t N, int32_t X, int32_t Y, int32_t Z, const float* __restrict__ tsdf, const float* __restrict__ level,
                    uint32_t* __restrict__ counts)
{
    const int64_t n = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    if (n >= N) return;
    int32_t ijk[3];
    float a, b[3];
    counts[n] = __popc(fus_edges(n, X, Y, Z, tsdf, *level, ijk, &a, b));
}

struct FusOrigin {
    double o[3];
};

__global__ void __launch_bounds__(FUS_THREADS)
fusion_extract_kernel(int64_t N, int32_t X, int32_t Y, int32_t Z, const float* __restrict__ tsdf, const float* __restrict__ color,
                      const float* __restrict__ level_ptr, const uint32_t* __restrict__ offsets, int64_t M, float voxel_size,
                      FusOrigin origin, float* __restrict__ verts, double* __restrict__ points, int64_t* __restrict__ index,
                      uint8_t* __restrict__ colors)
{
    const int64_t n = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    if (n >= N) return;
    int32_t ijk[3];
    float a, b[3];
    const float level = *level_ptr;
    const uint32_t bits = fus_edges(n, X, Y, Z, tsdf, level, ijk, &a, b);
    if (!bits) return;
    int64_t m = offsets[n];
    const int64_t stride[3] = {(int64_t)Y * Z, (int64_t)Z, 1};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!(bits & (1u << ax))) continue;
        if (m >= M) return;   // never with the M the count pass returned
        const float v = (float)ijk[ax] + (level - a) / (b[ax] - a);
        int32_t r = ijk[ax];
        if (v == v) r = (int32_t)rintf(v);
        r = min(max(r, ijk[ax]), ijk[ax] + 1);   // a crossing vertex lies on its edge: rint picks one of its two ends
        const int64_t src = n + (int64_t)(r - ijk[ax]) * stride[ax];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float vk = k == ax ? v : (float)ijk[k];
            verts[m * 3 + k] = vk;
            points[m * 3 + k] = (double)(vk * voxel_size) + origin.o[k];
            const float c = floorf(color[src * 3 + k]);
            colors[m * 3 + k] = (uint8_t)(c < 0.f ? 0.f : (c > 255.f ? 255.f : c));
        }
        index[m] = src;
        ++m;
    }
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_gather_kernel(int64_t M, int64_t N, int32_t C, const float* __restrict__ feat, const int64_t* __restrict__ index,
                     float* __restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t m = (int64_t)blockIdx.x * (FUS_THREADS / WAVE) + threadIdx.x / WAVE;
    if (m >= M || lane * 4 >= C) return;
    const int64_t src = index[m];
    if (src < 0 || src >= N) return;   // an M above the counted total leaves index rows unwritten: never follow them
    reinterpret_cast<float4*>(out + m * C)[lane] = reinterpret_cast<const float4*>(feat + src * C)[lane];
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_fusion_bytes(int32_t X, int32_t Y, int32_t Z, int32_t C, size_t* volume_bytes, size_t* surface_bytes)
{
    if (volume_bytes) *volume_bytes = 0;
    if (surface_bytes) *surface_bytes = 0;
    if (X < 1 || Y < 1 || Z < 1 || !volume_bytes || !surface_bytes) return SPLATRASTER_ERR_BAD_ARG;
    if ((int64_t)X * Y > FUS_MAX_VOXELS || (int64_t)X * Y * Z > FUS_MAX_VOXELS) return SPLATRASTER_ERR_BAD_ARG;
    if (C < 4 || C > FUS_MAX_FEAT || C % 4) return SPLATRASTER_ERR_BAD_ARG;
    const size_t N = (size_t)X * Y * Z;
    *volume_bytes = N * sizeof(float) * (size_t)(1 + 1 + 3 + C);
    *surface_bytes = fus_layout(nullptr, (int64_t)N).bytes;
    return SPLATRASTER_OK;
}

int splatraster_fusion_integrate(const splatraster_fusion_volume* v, int32_t F, int32_t H, int32_t W, const float* depth,
                                 const float* color_im, const float* feat_im, const float* world2cam, const float* intrinsics,
                                 float obs_weight, float sdf_trunc, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (bad_volume(v, true) || !v->axis[0] || !v->axis[1] || !v->axis[2]) return SPLATRASTER_ERR_BAD_ARG;
    if (F < 0 || F > FUS_MAX_FRAMES || H < 1 || W < 1 || H > FUS_MAX_IMAGE || W > FUS_MAX_IMAGE) return SPLATRASTER_ERR_BAD_ARG;
    if (F == 0) return SPLATRASTER_OK;
    if (!depth || !color_im || !feat_im || !world2cam || !intrinsics) return SPLATRASTER_ERR_BAD_ARG;
    if (misaligned(feat_im, 16)) return SPLATRASTER_ERR_BAD_ARG;
    if (!(sdf_trunc > 0.f) || obs_weight != obs_weight) return SPLATRASTER_ERR_BAD_ARG;
    FusFrames fr;
    for (int f = 0; f < FUS_MAX_FRAMES; ++f) {
        for (int k = 0; k < 12; ++k) fr.w2c[f][k] = f < F ? world2cam[f * 12 + k] : 0.f;
        for (int k = 0; k < 4; ++k) fr.intr[f][k] = f < F ? intrinsics[f * 4 + k] : 0.f;
    }
    const int64_t N = (int64_t)v->dim[0] * v->dim[1] * v->dim[2];
    const unsigned nb = (unsigned)((N + FUS_THREADS - 1) / FUS_THREADS);
    hipLaunchKernelGGL(fusion_integrate_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, N, v->dim[1], v->dim[2], v->feat_dim,
                       v->axis[0], v->axis[1], v->axis[2], v->tsdf, v->weight, v->color, v->feat, F, H, W, depth, color_im, feat_im,
                       fr, obs_weight, sdf_trunc);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_fusion_surface_count(const splatraster_fusion_volume* v, int32_t use_level, float level, void* workspace,
                                     int64_t* n_vertices, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (n_vertices) *n_vertices = 0;
    if (bad_volume(v, false) || !workspace || !n_vertices || (use_level && level != level)) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t N = (int64_t)v->dim[0] * v->dim[1] * v->dim[2];
    const FusWs w = fus_layout(workspace, N);
    const unsigned nb = (unsigned)((N + FUS_THREADS - 1) / FUS_THREADS);
    if (use_level) {
        hipLaunchKernelGGL(fusion_set_level_kernel, dim3(1), dim3(1), 0, stream, level, w.level);
        SR_LAUNCH_CHECK();
    } else {
        const int G = (int)(nb < (unsigned)FUS_MINMAX_BLOCKS ? nb : (unsigned)FUS_MINMAX_BLOCKS);
        hipLaunchKernelGGL(fusion_minmax_kernel, dim3(G), dim3(FUS_THREADS), 0, stream, N, v->tsdf, w.partial);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(fusion_level_kernel, dim3(1), dim3(FUS_THREADS), 0, stream, G, w.partial, w.level);
        SR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fusion_count_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, N, v->dim[0], v->dim[1], v->dim[2], v->tsdf,
                       w.level, w.counts);
    SR_LAUNCH_CHECK();
    const int st = exclusive_scan_u32(N, w.counts, reinterpret_cast<uint32_t*>(w.total), w.scan_tmp, stream, false);
    if (st != SPLATRASTER_OK) return st;
    uint64_t total = 0;
    SR_HIP_CHECK(hipMemcpyAsync(&total, w.total, sizeof(total), hipMemcpyDeviceToHost, stream));
    SR_HIP_CHECK(hipStreamSynchronize(stream));
    *n_vertices = (int64_t)total;
    return SPLATRASTER_OK;
}

int splatraster_fusion_surface_extract(const splatraster_fusion_volume* v, const void* workspace, double voxel_size,
                                       const double* origin, int64_t M, float* verts, double* points, int64_t* index,
                                       uint8_t* colors, float* feats, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (bad_volume(v, true) || !workspace || !origin || M < 0) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t N = (int64_t)v->dim[0] * v->dim[1] * v->dim[2];
    if (M > 3 * N) return SPLATRASTER_ERR_BAD_ARG;
    const FusWs w = fus_layout(const_cast<void*>(workspace), N);
    if (M == 0) return SPLATRASTER_OK;
    if (!verts || !points || !index || !colors || !feats || misaligned(feats, 16)) return SPLATRASTER_ERR_BAD_ARG;
    FusOrigin o;
    for (int k = 0; k < 3; ++k) o.o[k] = origin[k];
    SR_HIP_CHECK(hipMemsetAsync(index, 0xFF, (size_t)M * sizeof(int64_t), stream));   // -1: rows the write pass does not reach
    const unsigned nb = (unsigned)((N + FUS_THREADS - 1) / FUS_THREADS);
    hipLaunchKernelGGL(fusion_extract_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, N, v->dim[0], v->dim[1], v->dim[2], v->tsdf,
                       v->color, w.level, w.counts, M, (float)voxel_size, o, verts, points, index, colors);
    SR_LAUNCH_CHECK();
    const int per = FUS_THREADS / WAVE;
    hipLaunchKernelGGL(fusion_gather_kernel, dim3((unsigned)((M + per - 1) / per)), dim3(FUS_THREADS), 0, stream, M, N, v->feat_dim,
                       v->feat, index, feats);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
