// fusion.h — what the translation units of the feature-TSDF fusion share (fusion.hip: integration and surface vertices;
// fusion_mesh.hip: faces and normals over those vertices): the limits, the argument check, the surface workspace and the edge
// test that decides which grid edges own a vertex.
#pragma once
#include "common.h"

#include <math.h>

namespace sr {

constexpr int FUS_THREADS = 256;
constexpr int FUS_MAX_FRAMES = SPLATRASTER_FUSION_MAX_FRAMES;
constexpr int FUS_MAX_FEAT = SPLATRASTER_FUSION_MAX_FEAT_DIM;
constexpr int64_t FUS_MAX_VOXELS = (int64_t)1 << 30;   // 3 edges per voxel stay below 2^32 in the u32 scan
constexpr int FUS_MAX_IMAGE = 32768;                    // H, W: a pixel index fits an int, (float)W is exact
constexpr int FUS_MINMAX_BLOCKS = 1024;

static inline bool bad_volume(const splatraster_fusion_volume* v, bool need_feat)
{
    if (!v) return true;
    if (v->dim[0] < 1 || v->dim[1] < 1 || v->dim[2] < 1) return true;
    if ((int64_t)v->dim[0] * v->dim[1] > FUS_MAX_VOXELS || (int64_t)v->dim[0] * v->dim[1] * v->dim[2] > FUS_MAX_VOXELS) return true;
    if (v->feat_dim < 4 || v->feat_dim > FUS_MAX_FEAT || v->feat_dim % 4) return true;
    if (!v->tsdf || !v->weight || !v->color) return true;
    if (need_feat && (!v->feat || misaligned(v->feat, 16))) return true;
    return false;
}

// ---- surface workspace --------------------------------------------------------------------------------------------------
// [level, total | counts N | min/max partials | scan state]; level and total share the first section, at +0 and +128
struct FusWs {
    float* level;
    uint64_t* total;
    uint32_t* counts;
    float* partial;
    void* scan_tmp;
    size_t bytes;
};

static inline FusWs fus_layout(void* workspace, int64_t N)
{
    FusWs w;
    Carver c{workspace};
    char* head = c.take<char>(256);
    w.level = reinterpret_cast<float*>(head);
    w.total = head ? reinterpret_cast<uint64_t*>(head + 128) : nullptr;
    w.counts = c.take<uint32_t>((size_t)N);
    w.partial = c.take<float>(2 * FUS_MINMAX_BLOCKS);
    w.scan_tmp = c.take<char>(scan_tmp_bytes(N));
    w.bytes = c.o;
    return w;
}

__device__ __forceinline__ bool fus_cross(float a, float b, float level) { return (a < level) != (b < level); }

// the +x, +y, +z neighbours of voxel n that exist, and which of the three edges cross the level (bit a: axis a)
__device__ __forceinline__ uint32_t fus_edges(int64_t n, int32_t X, int32_t Y, int32_t Z, const float* __restrict__ tsdf, float level,
                                              int32_t* ijk, float* a, float* b)
{
    const int64_t YZ = (int64_t)Y * Z;
    const int32_t x = (int32_t)(n / YZ);
    const int32_t r = (int32_t)(n - (int64_t)x * YZ);
    const int32_t y = r / Z;
    const int32_t z = r - y * Z;
    ijk[0] = x;
    ijk[1] = y;
    ijk[2] = z;
    *a = tsdf[n];
    uint32_t bits = 0;
    b[0] = b[1] = b[2] = 0.f;
    if (x + 1 < X) {
        b[0] = tsdf[n + YZ];
        bits |= fus_cross(*a, b[0], level) ? 1u : 0u;
    }
    if (y + 1 < Y) {
        b[1] = tsdf[n + Z];
        bits |= fus_cross(*a, b[1], level) ? 2u : 0u;
    }
    if (z + 1 < Z) {
        b[2] = tsdf[n + 1];
        bits |= fus_cross(*a, b[2], level) ? 4u : 0u;
    }
    return bits;
}

}  // namespace sr
