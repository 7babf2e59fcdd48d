// fusion_mesh.hip — the triangles and vertex normals of the TSDF's level set over the vertices of fusion.hip's surface pass
// (get_mesh of utils/fusion_utils.py:271-289; the triangulation and the normal rule are the project's own).  Definition:
// include/splatraster.h (splatraster_fusion_mesh_*) and INTEGRATION.md §20; the table: fusion_mesh.h.
//
// gfx950 shape.  The stage reads the TSDF only (4 bytes per voxel), never the colour or feature volumes.  Faces: one lane per
// cell in linear [X-1, Y-1, Z-1] order, consecutive lanes along z as the volume is laid out, so the eight corner loads of a wave
// are four pairs of contiguous rows.  A count pass (case -> triangle count from the __constant__ table), exclusive_scan_u32, and a
// write pass that recomputes the case.  The vertex of edge (owner voxel n', axis) is offsets[n'] + popc(bits(n') & ((1 << axis) -
// 1)) with the surface pass's scanned counts; the owner's lower crossing bits are re-read from the TSDF (its +x / +y neighbour
// may lie outside the cell), not kept per voxel: only cells the surface passes through get that far, their extra loads fall into
// rows the wave or its neighbours have just loaded, and a byte per voxel would add a quarter to the traffic of a pass that is
// bound by the 4 bytes per voxel it must read.  Normals: one lane per voxel, the walk of fusion_extract_kernel.
// Compiled without FP contraction: every operation rounds on its own, in the order written.
#include "fusion.h"
#include "fusion_mesh.h"

namespace sr {

constexpr McTable MC_TABLE_HOST = make_mc_table();
__constant__ McTable MC_TABLE = make_mc_table();

static_assert(mc_total_triangles(MC_TABLE_HOST) == 820, "the derived table has 820 triangles");
static_assert(MC_TABLE_HOST.b[0x00][0] == 0 && MC_TABLE_HOST.b[0xFF][0] == 0, "no triangle without a crossing");
static_assert(MC_TABLE_HOST.b[0x01][0] == 1 && MC_TABLE_HOST.b[0x01][1] == 0 && MC_TABLE_HOST.b[0x01][2] == 4
                  && MC_TABLE_HOST.b[0x01][3] == 8 && MC_TABLE_HOST.b[0x01][4] == 0xFF,
              "case 0x01 is the triangle (0, 4, 8)");
static_assert(sizeof(McTable) == 4096 && MC_ROW == sizeof(uint4), "a case's row is 16 bytes, 16-byte aligned");

constexpr int64_t MESH_MAX_CELLS = (int64_t)UINT32_MAX / MC_MAX_TRIANGLES;   // 5 triangles per cell stay below 2^32 in the scan

// [total | counts cells | scan state]
struct MeshWs {
    uint64_t* total;
    uint32_t* counts;
    void* scan_tmp;
    size_t bytes;
};

static MeshWs mesh_layout(void* workspace, int64_t cells)
{
    MeshWs w;
    Carver c{workspace};
    w.total = c.take<uint64_t>(1);
    w.counts = c.take<uint32_t>((size_t)cells);
    w.scan_tmp = c.take<char>(scan_tmp_bytes(cells > 0 ? cells : 1));
    w.bytes = c.o;
    return w;
}

static int64_t mesh_cells(int32_t X, int32_t Y, int32_t Z) { return (int64_t)(X - 1) * (Y - 1) * (Z - 1); }

// cell c in linear [X-1, Y-1, Z-1] order: its lowest voxel's coordinates and linear index, and its case (bit c: corner c below)
__device__ __forceinline__ uint32_t mesh_case(int64_t c, int32_t Y, int32_t Z, const float* __restrict__ tsdf, float level, int32_t* ijk,
                                              int64_t* n0)
{
    const int64_t cyz = (int64_t)(Y - 1) * (Z - 1);
    const int32_t x = (int32_t)(c / cyz);
    const int32_t r = (int32_t)(c - (int64_t)x * cyz);
    const int32_t y = r / (Z - 1);
    const int32_t z = r - y * (Z - 1);
    ijk[0] = x;
    ijk[1] = y;
    ijk[2] = z;
    const int64_t YZ = (int64_t)Y * Z;
    const int64_t n = (int64_t)x * YZ + (int64_t)y * Z + z;
    *n0 = n;
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) bits |= (tsdf[n + (k & 1) * YZ + ((k >> 1) & 1) * Z + (k >> 2)] < level ? 1u : 0u) << k;
    return bits;
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_mesh_count_kernel(int64_t cells, int32_t Y, int32_t Z, const float* __restrict__ tsdf, const float* __restrict__ level,
                         uint32_t* __restrict__ counts)
{
    const int64_t c = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    if (c >= cells) return;
    int32_t ijk[3];
    int64_t n0;
    counts[c] = MC_TABLE.b[mesh_case(c, Y, Z, tsdf, *level, ijk, &n0)][0];
}

// vertex id of edge e of the cell at (ijk, n0): the owner is the corner the edge starts at
__device__ __forceinline__ int32_t mesh_vertex(uint32_t e, const int32_t* ijk, int64_t n0, int32_t X, int32_t Y, int32_t Z,
                                               const float* __restrict__ tsdf, float level, const uint32_t* __restrict__ voffsets)
{
    const uint32_t axis = e >> 2, k = e & 3;
    const uint32_t start = axis == 0 ? (k << 1) : (axis == 1 ? ((k & 1) | ((k >> 1) << 2)) : k);
    const int64_t YZ = (int64_t)Y * Z;
    const int64_t n = n0 + (start & 1) * YZ + ((start >> 1) & 1) * Z + (start >> 2);
    uint32_t id = voffsets[n];
    if (axis >= 1) {
        const float a = tsdf[n];
        if (ijk[0] + (int32_t)(start & 1) + 1 < X) id += fus_cross(a, tsdf[n + YZ], level) ? 1u : 0u;
        if (axis == 2 && ijk[1] + (int32_t)((start >> 1) & 1) + 1 < Y) id += fus_cross(a, tsdf[n + Z], level) ? 1u : 0u;
    }
    return (int32_t)id;
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_mesh_faces_kernel(int64_t cells, int32_t X, int32_t Y, int32_t Z, const float* __restrict__ tsdf,
                         const float* __restrict__ level_ptr, const uint32_t* __restrict__ voffsets,
                         const uint32_t* __restrict__ foffsets, int64_t F, int32_t* __restrict__ faces)
{
    const int64_t c = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    if (c >= cells) return;
    int32_t ijk[3];
    int64_t n0;
    const float level = *level_ptr;
    const uint32_t cs = mesh_case(c, Y, Z, tsdf, level, ijk, &n0);
    // one global_load_dwordx4: left as a plain uint4 load the compiler narrows it to a byte and three words
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 row = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(MC_TABLE.b[cs]));
    const uint32_t count = row.x & 0xFF;
    if (!count) return;
    const uint32_t words[4] = {row.x, row.y, row.z, row.w};
    int64_t f = foffsets[c];
#pragma unroll
    for (int t = 0; t < MC_MAX_TRIANGLES; ++t) {
        if ((uint32_t)t >= count) return;
        if (f >= F) return;   // never with the F the count pass returned
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int byte = 1 + 3 * t + j;
            const uint32_t e = (words[byte >> 2] >> (8 * (byte & 3))) & 0xFF;
            faces[f * 3 + j] = mesh_vertex(e, ijk, n0, X, Y, Z, tsdf, level, voffsets);
        }
        ++f;
    }
}

// central difference of the TSDF at voxel n = (ijk), one-sided at the two ends of an axis, 0 on an axis of one voxel
__device__ __forceinline__ void mesh_gradient(const float* __restrict__ tsdf, int64_t n, const int32_t* ijk, const int32_t* dim,
                                              const int64_t* stride, float* g)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dim[k] < 2)
            g[k] = 0.f;
        else if (ijk[k] == 0)
            g[k] = tsdf[n + stride[k]] - tsdf[n];
        else if (ijk[k] == dim[k] - 1)
            g[k] = tsdf[n] - tsdf[n - stride[k]];
        else
            g[k] = 0.5f * (tsdf[n + stride[k]] - tsdf[n - stride[k]]);
    }
}

__global__ void __launch_bounds__(FUS_THREADS)
fusion_mesh_normals_kernel(int64_t N, int32_t X, int32_t Y, int32_t Z, const float* __restrict__ tsdf,
                           const float* __restrict__ level_ptr, const uint32_t* __restrict__ offsets, int64_t M,
                           float* __restrict__ normals)
{
    const int64_t n = (int64_t)blockIdx.x * FUS_THREADS + threadIdx.x;
    if (n >= N) return;
    int32_t ijk[3];
    float a, b[3];
    const float level = *level_ptr;
    const uint32_t bits = fus_edges(n, X, Y, Z, tsdf, level, ijk, &a, b);
    if (!bits) return;
    int64_t m = offsets[n];
    const int32_t dim[3] = {X, Y, Z};
    const int64_t stride[3] = {(int64_t)Y * Z, (int64_t)Z, 1};
    float ga[3];
    mesh_gradient(tsdf, n, ijk, dim, stride, ga);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!(bits & (1u << ax))) continue;
        if (m >= M) return;   // never with the M the count pass returned
        int32_t nb[3] = {ijk[0], ijk[1], ijk[2]};
        nb[ax] += 1;
        float gb[3];
        mesh_gradient(tsdf, n + stride[ax], nb, dim, stride, gb);
        const float q = (level - a) / (b[ax] - a);
        const float g0 = ga[0] + q * (gb[0] - ga[0]);
        const float g1 = ga[1] + q * (gb[1] - ga[1]);
        const float g2 = ga[2] + q * (gb[2] - ga[2]);
        const float len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
        const bool ok = len > 0.f && len < INFINITY;
        normals[m * 3 + 0] = ok ? g0 / len : 0.f;
        normals[m * 3 + 1] = ok ? g1 / len : 0.f;
        normals[m * 3 + 2] = ok ? g2 / len : 0.f;
        ++m;
    }
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_debug_mc_table(uint8_t* out)
{
    if (!out) return SPLATRASTER_ERR_BAD_ARG;
    for (int cs = 0; cs < 256; ++cs)
        for (int k = 0; k < MC_ROW; ++k) out[cs * MC_ROW + k] = MC_TABLE_HOST.b[cs][k];
    return SPLATRASTER_OK;
}

int splatraster_fusion_mesh_bytes(int32_t X, int32_t Y, int32_t Z, size_t* mesh_bytes)
{
    if (mesh_bytes) *mesh_bytes = 0;
    if (X < 1 || Y < 1 || Z < 1 || !mesh_bytes) return SPLATRASTER_ERR_BAD_ARG;
    if ((int64_t)X * Y > FUS_MAX_VOXELS || (int64_t)X * Y * Z > FUS_MAX_VOXELS) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t cells = mesh_cells(X, Y, Z);
    if (cells > MESH_MAX_CELLS) return SPLATRASTER_ERR_OVERFLOW;
    *mesh_bytes = mesh_layout(nullptr, cells).bytes;
    return SPLATRASTER_OK;
}

int splatraster_fusion_mesh_count(const splatraster_fusion_volume* v, const void* surface_workspace, void* mesh_workspace,
                                  int64_t* n_faces, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (n_faces) *n_faces = 0;
    if (bad_volume(v, false) || !surface_workspace || !mesh_workspace || !n_faces) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t N = (int64_t)v->dim[0] * v->dim[1] * v->dim[2];
    const int64_t cells = mesh_cells(v->dim[0], v->dim[1], v->dim[2]);
    if (cells > MESH_MAX_CELLS) return SPLATRASTER_ERR_OVERFLOW;
    const FusWs s = fus_layout(const_cast<void*>(surface_workspace), N);
    const MeshWs w = mesh_layout(mesh_workspace, cells);
    if (cells > 0) {
        const unsigned nb = (unsigned)((cells + FUS_THREADS - 1) / FUS_THREADS);
        hipLaunchKernelGGL(fusion_mesh_count_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, cells, v->dim[1], v->dim[2], v->tsdf,
                           s.level, w.counts);
        SR_LAUNCH_CHECK();
        const int st = exclusive_scan_u32(cells, w.counts, reinterpret_cast<uint32_t*>(w.total), w.scan_tmp, stream, false);
        if (st != SPLATRASTER_OK) return st;
    }
    uint64_t totals[2] = {0, 0};   // vertices (of the surface count), faces
    SR_HIP_CHECK(hipMemcpyAsync(&totals[0], s.total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (cells > 0) SR_HIP_CHECK(hipMemcpyAsync(&totals[1], w.total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SR_HIP_CHECK(hipStreamSynchronize(stream));
    if (totals[0] > (uint64_t)INT32_MAX || totals[1] > (uint64_t)INT32_MAX) return SPLATRASTER_ERR_OVERFLOW;   // PLY int faces
    *n_faces = (int64_t)totals[1];
    return SPLATRASTER_OK;
}

int splatraster_fusion_mesh_extract(const splatraster_fusion_volume* v, const void* surface_workspace, const void* mesh_workspace,
                                    int64_t M, int64_t F, int32_t* faces, float* normals, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (bad_volume(v, false) || !surface_workspace || !mesh_workspace || M < 0 || F < 0) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t N = (int64_t)v->dim[0] * v->dim[1] * v->dim[2];
    const int64_t cells = mesh_cells(v->dim[0], v->dim[1], v->dim[2]);
    if (cells > MESH_MAX_CELLS) return SPLATRASTER_ERR_OVERFLOW;
    if (M > 3 * N || F > MC_MAX_TRIANGLES * cells || M > INT32_MAX || F > INT32_MAX) return SPLATRASTER_ERR_BAD_ARG;
    if ((M > 0 && !normals) || (F > 0 && !faces)) return SPLATRASTER_ERR_BAD_ARG;
    const FusWs s = fus_layout(const_cast<void*>(surface_workspace), N);
    const MeshWs w = mesh_layout(const_cast<void*>(mesh_workspace), cells);
    if (F > 0) {
        SR_HIP_CHECK(hipMemsetAsync(faces, 0xFF, (size_t)F * 3 * sizeof(int32_t), stream));   // -1: rows the write pass does not reach
        const unsigned nb = (unsigned)((cells + FUS_THREADS - 1) / FUS_THREADS);
        hipLaunchKernelGGL(fusion_mesh_faces_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, cells, v->dim[0], v->dim[1], v->dim[2],
                           v->tsdf, s.level, s.counts, w.counts, F, faces);
        SR_LAUNCH_CHECK();
    }
    if (M > 0) {
        const unsigned nb = (unsigned)((N + FUS_THREADS - 1) / FUS_THREADS);
        hipLaunchKernelGGL(fusion_mesh_normals_kernel, dim3(nb), dim3(FUS_THREADS), 0, stream, N, v->dim[0], v->dim[1], v->dim[2],
                           v->tsdf, s.level, s.counts, M, normals);
        SR_LAUNCH_CHECK();
    }
    return SPLATRASTER_OK;
}

}  // extern "C"
