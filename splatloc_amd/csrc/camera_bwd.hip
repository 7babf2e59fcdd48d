// camera_bwd.hip — the camera gradients of the V views of a window, and nothing else (splatraster_backward_window_cameras:
// pose refinement of a window of query frames against a frozen map, splatloc_amd/pose.py refine_poses).
//
// One thread per (view, Gaussian), grid (ceil(P / 256), V): a block never straddles two views.  A thread reads what
// preprocess_bwd_kernel<true> reads of that row — the forward's record, the moments the compositing backward left in the view's
// accumulator row, the view's camera — and forms the same 27 partials (preprocess_bwd.hip: dV[4c + r], r < 3; dPM[4c + k],
// k = 0, 1, 3; the three dcampos terms, zero here: a window has precomputed colours only).  No per-Gaussian gradient, no
// dL/dmeans2D is stored: the kernel writes 35 floats per view.
// The per-row derivative is this file's own copy of preprocess_bwd.hip's, cut down to the terms the camera needs (no Sigma3,
// scale, quaternion, mean or opacity chain): preprocess_bwd_kernel's text and code generation stay what they were.
// The reduction is that kernel's: wave_reduce_pack<27>, the four waves in LDS, one returning atomic per value and block into set
// blockIdx.x % POSE_SETS of the block's OWN view, a two-level ticket per view; the view's last block sums its sets and writes
// all 16 + 16 + 3 entries.  Nothing waits for another block.
#include "composite_common.h"

namespace sr {

constexpr int CAM_WS_FLOATS = (int)(POSE_ACC_BYTES / sizeof(float));   // per view: POSE_SETS sets + the ticket's line

__global__ void __launch_bounds__(256)
camera_bwd_kernel(int P, int W, int H, float mod, WinCams cams, const float* __restrict__ means3D,
                  const float* __restrict__ scales, const float* __restrict__ rotations,
                  const float* __restrict__ cov3D_precomp, const float4* __restrict__ rec, const float* __restrict__ gacc,
                  GaccLayout GL, int MO, float* __restrict__ ws, float* __restrict__ dL_dview, float* __restrict__ dL_dproj,
                  float* __restrict__ dL_dcampos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    float pose[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) pose[k] = 0.f;
    if (i < P && cams.radii[v][i] > 0) {
        const float* __restrict__ view = cams.view[v];
        const float* __restrict__ proj = cams.proj[v];
        const float tanfovx = cams.tanfovx[v], tanfovy = cams.tanfovy[v];
        float Vm[16], PM[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { Vm[k] = view[k]; PM[k] = proj[k]; }
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        // 3D covariance (recomputed; same formula as the forward)
        float c6[6];
        if (cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * i + k];
        } else {
            const float4 qv = reinterpret_cast<const float4*>(rotations)[i];
            const float r = qv.x, x = qv.y, y = qv.z, z = qv.w;
            const float Rm[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                                    {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                                    {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
            const float sc[3] = {mod * scales[3 * i], mod * scales[3 * i + 1], mod * scales[3 * i + 2]};
            float L[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) L[j][k] = Rm[j][k] * sc[k];
            c6[0] = L[0][0] * L[0][0] + L[0][1] * L[0][1] + L[0][2] * L[0][2];
            c6[1] = L[0][0] * L[1][0] + L[0][1] * L[1][1] + L[0][2] * L[1][2];
            c6[2] = L[0][0] * L[2][0] + L[0][1] * L[2][1] + L[0][2] * L[2][2];
            c6[3] = L[1][0] * L[1][0] + L[1][1] * L[1][1] + L[1][2] * L[1][2];
            c6[4] = L[1][0] * L[2][0] + L[1][1] * L[2][1] + L[1][2] * L[2][2];
            c6[5] = L[2][0] * L[2][0] + L[2][1] * L[2][1] + L[2][2] * L[2][2];
        }
        const float S3[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
        const size_t gr = (size_t)v * P + i;   // row of (view, Gaussian)
        const float* mrow = gacc + GL.index(gr, (size_t)i, (uint32_t)MO);  // moment record of this row
        const float4 g0 = make_float4(mrow[0], mrow[1], mrow[2], mrow[3]);
        const float g1x = mrow[4], gdepth = mrow[6];
        const float4 con = rec[2 * gr + 1];  // conic a, b, c, opacity of the forward
        // power = -1/2 (A dx^2 + C dy^2) - B dx dy, alpha = o G:
        const float dm2x = -0.5f * (float)W * con.w * (con.x * g0.x + con.y * g0.y);
        const float dm2y = -0.5f * (float)H * con.w * (con.z * g0.y + con.y * g0.x);
        const float gA = -0.5f * con.w * g0.z, gB = -con.w * g0.w, gC = -0.5f * con.w * g1x;
        const float tx0 = Vm[0] * px + Vm[4] * py + Vm[8] * pz + Vm[12];
        const float ty0 = Vm[1] * px + Vm[5] * py + Vm[9] * pz + Vm[13];
        const float tz = Vm[2] * px + Vm[6] * py + Vm[10] * pz + Vm[14];
        const float focal_x = (float)W / (2.0f * tanfovx), focal_y = (float)H / (2.0f * tanfovy);
        const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
        const float txtz = tx0 / tz, tytz = ty0 / tz;
        const float xg = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
        const float yg = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
        const float ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
        const float itz = 1.0f / tz, itz2 = itz * itz, itz3 = itz2 * itz;
        const float J00 = focal_x * itz, J02 = -(focal_x * tx) * itz2;
        const float J11 = focal_y * itz, J12 = -(focal_y * ty) * itz2;
        // Wv[r][c] = V[4c + r]
        float A0[3], A1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A0[c] = J00 * Vm[4 * c + 0] + J02 * Vm[4 * c + 2];
            A1[c] = J11 * Vm[4 * c + 1] + J12 * Vm[4 * c + 2];
        }
        float SA0[3], SA1[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            SA0[j] = S3[j][0] * A0[0] + S3[j][1] * A0[1] + S3[j][2] * A0[2];
            SA1[j] = S3[j][0] * A1[0] + S3[j][1] * A1[1] + S3[j][2] * A1[2];
        }
        const float a = A0[0] * SA0[0] + A0[1] * SA0[1] + A0[2] * SA0[2] + DILATION;
        const float b = A0[0] * SA1[0] + A0[1] * SA1[1] + A0[2] * SA1[2];
        const float c = A1[0] * SA1[0] + A1[1] * SA1[1] + A1[2] * SA1[2] + DILATION;
        const float det = a * c - b * b;
        float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
        if (det != 0.f) {
            const float d2 = 1.0f / (det * det);
            dL_da = (-c * c * gA + b * c * gB - b * b * gC) * d2;
            dL_db = (2.f * b * c * gA - (det + 2.f * b * b) * gB + 2.f * a * b * gC) * d2;
            dL_dc = (-b * b * gA + a * b * gB - a * a * gC) * d2;
        }
        const float G2[2][2] = {{dL_da, 0.5f * dL_db}, {0.5f * dL_db, dL_dc}};
        // dL/dJ = 2 G2 J Sigma_v with J Sigma_v = (A Sigma3) Wv^T ; (A Sigma3)[r][k] = SA_r[k]
        float JS0[3], JS1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            JS0[k] = SA0[0] * Vm[0 + k] + SA0[1] * Vm[4 + k] + SA0[2] * Vm[8 + k];
            JS1[k] = SA1[0] * Vm[0 + k] + SA1[1] * Vm[4 + k] + SA1[2] * Vm[8 + k];
        }
        const float dJ00 = 2.f * (G2[0][0] * JS0[0] + G2[0][1] * JS1[0]);
        const float dJ02 = 2.f * (G2[0][0] * JS0[2] + G2[0][1] * JS1[2]);
        const float dJ11 = 2.f * (G2[1][0] * JS0[1] + G2[1][1] * JS1[1]);
        const float dJ12 = 2.f * (G2[1][0] * JS0[2] + G2[1][1] * JS1[2]);
        const float dtx = xg * (-focal_x * itz2 * dJ02);
        const float dty = yg * (-focal_y * itz2 * dJ12);
        const float dtz = -focal_x * itz2 * dJ00 - focal_y * itz2 * dJ11 + 2.f * focal_x * tx * itz3 * dJ02 +
                          2.f * focal_y * ty * itz3 * dJ12;
        // t = Wv p + trans (V[4c + r] multiplies p[c] into t[r]); cov2D = A Sigma3 A^T with
        // A = J Wv: dL/dA = 2 G2 A Sigma3, dL/dWv = J^T dL/dA
        const float dt[3] = {dtx, dty, dtz + gdepth};
        const float pp[3] = {px, py, pz};
        float dA0[3], dA1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dA0[k] = 2.f * (G2[0][0] * SA0[k] + G2[0][1] * SA1[k]);
            dA1[k] = 2.f * (G2[1][0] * SA0[k] + G2[1][1] * SA1[k]);
        }
        // J = [[J00, 0, J02], [0, J11, J12]]
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            pose[3 * cc + 0] = dt[0] * pp[cc] + J00 * dA0[cc];
            pose[3 * cc + 1] = dt[1] * pp[cc] + J11 * dA1[cc];
            pose[3 * cc + 2] = dt[2] * pp[cc] + J02 * dA0[cc] + J12 * dA1[cc];
        }
        pose[9] = dt[0];
        pose[10] = dt[1];
        pose[11] = dt[2];
        // NDC mean2D through the projection: d/d(hx, hy, hw)
        const float hx = PM[0] * px + PM[4] * py + PM[8] * pz + PM[12];
        const float hy = PM[1] * px + PM[5] * py + PM[9] * pz + PM[13];
        const float hw = PM[3] * px + PM[7] * py + PM[11] * pz + PM[15];
        const float mw = 1.0f / (hw + 0.0000001f);
        const float mul1 = hx * mw * mw, mul2 = hy * mw * mw;
        const float dh[3] = {dm2x * mw, dm2y * mw, -(mul1 * dm2x + mul2 * dm2y)};
        const float p4[4] = {px, py, pz, 1.f};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int j = 0; j < 3; ++j) pose[12 + 3 * cc + j] = dh[j] * p4[cc];
    }
    // the reduction of preprocess_bwd_kernel<true>, on the sets and tickets of THIS view
    float* __restrict__ acc = ws + (size_t)v * CAM_WS_FLOATS;
    __shared__ float s_pose[4][32];
    __shared__ bool s_last;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const float tot = wave_reduce_pack<27>(pose, lane);
    const int slot = (int)(__brev((unsigned)lane) >> 26);
    if (slot < 27) s_pose[w][slot] = tot;
    __syncthreads();
    if (threadIdx.x < 27) {
        const int k = threadIdx.x;
        const float sum = s_pose[0][k] + s_pose[1][k] + s_pose[2][k] + s_pose[3][k];
        const float before = atomicAdd(&acc[(blockIdx.x & (POSE_SETS - 1)) * POSE_SET_FLOATS + k], sum);
        asm volatile("" ::"v"(before));     // (returned: the addition is done at the memory side before the ticket below)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned q = blockIdx.x & (POSE_SETS - 1);
        const unsigned in_set = (gridDim.x - q + (POSE_SETS - 1)) / POSE_SETS;       // blocks of this view that add to set q
        const unsigned nsets = gridDim.x < (unsigned)POSE_SETS ? gridDim.x : (unsigned)POSE_SETS;
        unsigned* set_ticket = reinterpret_cast<unsigned*>(acc + q * POSE_SET_FLOATS + (POSE_SET_FLOATS - 1));
        unsigned* ticket = reinterpret_cast<unsigned*>(acc + POSE_SETS * POSE_SET_FLOATS);
        // release / acquire at agent scope on both tickets, as in preprocess_bwd_kernel: this block's additions happen-before
        // the winner's loads of the sets
        bool last = false;
        if (__hip_atomic_fetch_add(set_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_set - 1)
            last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nsets - 1;
        s_last = last;
    }
    __syncthreads();
    if (s_last && threadIdx.x < 35) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int e = threadIdx.x;      // output entry: dV[0..15], dPM[16..31], dcampos[32..34]
        int k = -1;                     // its partial (dV[4c + r], r < 3: 3c + r; dPM[4c + j], j = 0, 1, 3: 12 + 3c + (j == 3 ? 2 : j))
        if (e < 16) { if ((e & 3) < 3) k = 3 * (e >> 2) + (e & 3); }
        else if (e < 32) { const int j = (e - 16) & 3; if (j != 2) k = 12 + 3 * ((e - 16) >> 2) + (j == 3 ? 2 : j); }
        else k = 24 + (e - 32);
        float sum = 0.0f;
        if (k >= 0) {
            for (int q = 0; q < POSE_SETS; ++q)
                sum += __hip_atomic_load(&acc[q * POSE_SET_FLOATS + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (e < 16) dL_dview[16 * v + e] = sum;
        else if (e < 32) dL_dproj[16 * v + e - 16] = sum;
        else if (dL_dcampos) dL_dcampos[3 * v + e - 32] = sum;
    }
}

int launch_camera_bwd(const splatraster_settings& s, int32_t P, int32_t V, const WinCams& cams, const float* means3D,
                      const float* scales, const float* rotations, const float* cov3D_precomp, const float4* rec,
                      const float* gacc, int C, float* ws, float* dL_dview, float* dL_dproj, float* dL_dcampos, hipStream_t stream)
{
    if (P <= 0 || V < 1 || V > MAX_VIEWS || !ws || !dL_dview || !dL_dproj) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(camera_bwd_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)V), dim3(256), 0, stream, P, s.image_width,
                       s.image_height, s.scale_modifier, cams, means3D, scales, rotations, cov3D_precomp, rec, gacc,
                       gacc_layout(C, P), gacc_moment_offset(C), ws, dL_dview, dL_dproj, dL_dcampos);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr
