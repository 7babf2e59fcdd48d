// projection_bwd.h — the per-(view, Gaussian) backward of the projection, once: the straight-line pieces that
// preprocess_bwd_kernel, camera_bwd_kernel and window_joint_bwd_kernel are built from.  Every kernel keeps its own shell (its
// loops over Gaussians and views, what it loads when, the order of its stores); the arithmetic is here.
// These functions are inlined into translation units compiled with fp contraction on: the text of an expression decides which
// multiplies fuse, so operand order and statement structure are part of the results (HISTORY.md §19).
#pragma once
#include "composite_common.h"

namespace sr {

// 3D covariance of Gaussian i (recomputed; same formula as the forward) — view independent.  c6: its upper triangle; Rm, sc, qv:
// rotation matrix, modulated scales and quaternion it was built from, which sigma3_chain_bwd needs again — zeroed HERE when the
// covariance is precomputed: the callers declare all four without a value.
__device__ __forceinline__ void sigma3_build(int i, float mod, const float* __restrict__ scales,
                                             const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
                                             float (&c6)[6], float (&Rm)[3][3], float (&sc)[3], float4& qv)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Rm[j][0] = Rm[j][1] = Rm[j][2] = 0.f;
        sc[j] = 0.f;
    }
    qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * i + k];
    } else {
        qv = reinterpret_cast<const float4*>(rotations)[i];
        const float r = qv.x, x = qv.y, y = qv.z, z = qv.w;
        Rm[0][0] = 1.f - 2.f * (y * y + z * z); Rm[0][1] = 2.f * (x * y - r * z); Rm[0][2] = 2.f * (x * z + r * y);
        Rm[1][0] = 2.f * (x * y + r * z); Rm[1][1] = 1.f - 2.f * (x * x + z * z); Rm[1][2] = 2.f * (y * z - r * x);
        Rm[2][0] = 2.f * (x * z - r * y); Rm[2][1] = 2.f * (y * z + r * x); Rm[2][2] = 1.f - 2.f * (x * x + y * y);
        sc[0] = mod * scales[3 * i]; sc[1] = mod * scales[3 * i + 1]; sc[2] = mod * scales[3 * i + 2];
        float L[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) L[j][k] = Rm[j][k] * sc[k];
        // Sigma3 = L L^T: row a of L times row b.  The fusing is spelled out — what the compiler made of `L[a][0] * L[b][0] +
        // L[a][1] * L[b][1] + L[a][2] * L[b][2]` inside preprocess_bwd_kernel.  Left to the compiler, which of the first two
        // products is fused depends on the function the text is inlined from, and Sigma3's last bit with it (HISTORY.md §19)
        const auto rows = [&L](int a, int b) { return fmaf(L[a][2], L[b][2], fmaf(L[a][0], L[b][0], L[a][1] * L[b][1])); };
        c6[0] = rows(0, 0); c6[1] = rows(0, 1); c6[2] = rows(0, 2);
        c6[3] = rows(1, 1); c6[4] = rows(1, 2); c6[5] = rows(2, 2);
    }
}

// One visible (view, Gaussian) row: the 32-byte record of gradient moments at mrow and the forward's (conic, opacity) record,
// loaded here BEHIND the moments as the kernels always did (the order of the loads enters the compiler's operand order: §19),
// become dL/dmean2D (NDC; dm2x, dm2y), and are chained through conic -> cov2D -> J and the view-space mean, and through the
// projection, ADDING the row's part to dop, dmean (dL/dmean3D) and G3s (dL/dSigma3, full symmetric).  POSE: the row's camera
// partials as well — pose[3c + r] = dV[4c + r] (r < 3), pose[12 + 3c + (0, 1, 2)] = dPM[4c + (0, 1, 3)]; pose[24..26], the
// dcampos terms of SH colours, are the caller's.  A caller that wants the camera terms alone passes accumulators it throws
// away: the compiler drops what only feeds them.
template <bool POSE>
__device__ __forceinline__ void projection_row_bwd(int W, int H, const float (&Vm)[16], const float (&PM)[16], float tanfovx,
                                                   float tanfovy, float px, float py, float pz, const float (&S3)[3][3],
                                                   const float* __restrict__ mrow, const float4* __restrict__ conic_opacity,
                                                   float& dm2x, float& dm2y, float& dop, float (&dmean)[3], float (&G3s)[3][3], float (&pose)[27])
{
    const float4 g0 = make_float4(mrow[0], mrow[1], mrow[2], mrow[3]);
    const float4 g1 = make_float4(mrow[4], mrow[5], mrow[6], 0.f);
    const float4 con = *conic_opacity;  // conic a, b, c, opacity of the forward
    // power = -1/2 (A dx^2 + C dy^2) - B dx dy, alpha = o G:
    dm2x = -0.5f * (float)W * con.w * (con.x * g0.x + con.y * g0.y);
    dm2y = -0.5f * (float)H * con.w * (con.z * g0.y + con.y * g0.x);
    const float gA = -0.5f * con.w * g0.z, gB = -con.w * g0.w, gC = -0.5f * con.w * g1.x;
    dop += g1.y;
    const float gdepth = g1.z;
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
    // dL/dSigma3 (full symmetric) = A^T G2 A — linear in the view's contribution, chained to scale / quaternion
    // once after the caller's loop over the views (sigma3_chain_bwd)
    float GA0[3], GA1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        GA0[k] = G2[0][0] * A0[k] + G2[0][1] * A1[k];
        GA1[k] = G2[1][0] * A0[k] + G2[1][1] * A1[k];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) G3s[j][k] += A0[j] * GA0[k] + A1[j] * GA1[k];
    // dL/dJ = 2 G2 J Sigma_v with J Sigma_v = (A Sigma3) Wv^T ; (A Sigma3)[r][k] = SA_r[k]
    float JS0[3], JS1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // column k of Sigma_v side: sum_c SA[c] * Wv[k][c]
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
#pragma unroll
    for (int k = 0; k < 3; ++k)  // Wv^T [dtx dty dtz]: Wv[r][k] = V[4k + r]
        dmean[k] += Vm[4 * k + 0] * dtx + Vm[4 * k + 1] * dty + Vm[4 * k + 2] * (dtz + gdepth);
    if (POSE) {
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
        for (int c = 0; c < 3; ++c) {
            pose[3 * c + 0] = dt[0] * pp[c] + J00 * dA0[c];
            pose[3 * c + 1] = dt[1] * pp[c] + J11 * dA1[c];
            pose[3 * c + 2] = dt[2] * pp[c] + J02 * dA0[c] + J12 * dA1[c];
        }
        pose[9] = dt[0];
        pose[10] = dt[1];
        pose[11] = dt[2];
    }
    // NDC mean2D -> mean3D
    const float hx = PM[0] * px + PM[4] * py + PM[8] * pz + PM[12];
    const float hy = PM[1] * px + PM[5] * py + PM[9] * pz + PM[13];
    const float hw = PM[3] * px + PM[7] * py + PM[11] * pz + PM[15];
    const float mw = 1.0f / (hw + 0.0000001f);
    const float mul1 = hx * mw * mw, mul2 = hy * mw * mw;
    dmean[0] += (PM[0] * mw - PM[3] * mul1) * dm2x + (PM[1] * mw - PM[3] * mul2) * dm2y;
    dmean[1] += (PM[4] * mw - PM[7] * mul1) * dm2x + (PM[5] * mw - PM[7] * mul2) * dm2y;
    dmean[2] += (PM[8] * mw - PM[11] * mul1) * dm2x + (PM[9] * mw - PM[11] * mul2) * dm2y;
    if (POSE) {
        const float dh[3] = {dm2x * mw, dm2y * mw, -(mul1 * dm2x + mul2 * dm2y)};  // d/d(hx, hy, hw)
        const float p4[4] = {px, py, pz, 1.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 3; ++j) pose[12 + 3 * c + j] = dh[j] * p4[c];
    }
}

// dL/dSigma3 summed over the views (G3s) back to what Sigma3 was built from: dcov (precomputed covariance) or dscale and drot
// (Rm, sc, qv of sigma3_build).  The other output(s) are left as they are.
__device__ __forceinline__ void sigma3_chain_bwd(bool precomp, float mod, const float (&G3s)[3][3], const float (&Rm)[3][3],
                                                 const float (&sc)[3], const float4 qv, float (&dcov)[6], float (&dscale)[3],
                                                 float (&drot)[4])
{
    if (precomp) {
        dcov[0] = G3s[0][0]; dcov[1] = 2.f * G3s[0][1]; dcov[2] = 2.f * G3s[0][2];
        dcov[3] = G3s[1][1]; dcov[4] = 2.f * G3s[1][2]; dcov[5] = G3s[2][2];
    } else {
        // Sigma3 = L L^T, L = R diag(s)  =>  dL/dL = 2 G3 L
        float dR[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float ds = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float dLjk = 2.f * (G3s[j][0] * Rm[0][k] + G3s[j][1] * Rm[1][k] + G3s[j][2] * Rm[2][k]) * sc[k];
                ds += dLjk * Rm[j][k];
                dR[j][k] = dLjk * sc[k];
            }
            dscale[k] = ds * mod;
        }
        const float r = qv.x, x = qv.y, y = qv.z, z = qv.w;
        drot[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
        drot[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1] - 2.f * x * dR[2][2]);
        drot[2] = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1] - 2.f * y * dR[2][2]);
        drot[3] = 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
    }
}

// The camera sums of view v of a window (v = 0: a single view), called by EVERY thread of a 256-thread block with the 27 partials
// of its row (zeros for a thread without one).  They are summed over the wave with the packed butterfly, then over the block in
// LDS, then one atomic per value per block goes into set blockIdx.x % POSE_SETS of the view's slice of `ws` — per view POSE_SETS
// zeroed sets + the ticket line (common.h, POSE_ACC_FLOATS) — because every block on the same 27 words queued the atomics of
// 2 000 blocks on three lines: 13 us of the kernel at 500k Gaussians.  The last block of gridDim.x to take a ticket sums the sets
// and writes row v of the outputs ([V,16], [V,16], [V,3] or null), all 16 + 16 + 3 entries of it: nothing to zero beforehand but
// `ws`, and nothing waits for another block.
// s_pose and s_last are the one LDS allocation (516 bytes) of a kernel that calls this, however often: a following call writes
// s_pose behind this call's third barrier and s_last behind two more of its own.
// (ws, v and the output bases rather than the view's own pointers: formed before the call, those cost window_joint_bwd_kernel<4>
// seven registers and with them a wave per SIMD — HISTORY.md §19.)
__device__ __forceinline__ void camera_reduce(const float (&pose)[27], float* __restrict__ ws, int v, float* __restrict__ dL_dview,
                                              float* __restrict__ dL_dproj, float* __restrict__ dL_dcampos)
{
    float* __restrict__ acc = ws + (size_t)v * POSE_ACC_FLOATS;
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
    // two-level ticket (2 000 increments of ONE word would queue for ~40 us): the set's own counter in the last word of its
    // line, then — by the last block of every set — the counter behind the sets
    if (threadIdx.x == 0) {
        const unsigned q = blockIdx.x & (POSE_SETS - 1);
        const unsigned in_set = (gridDim.x - q + (POSE_SETS - 1)) / POSE_SETS;       // blocks that add to set q
        const unsigned nsets = gridDim.x < (unsigned)POSE_SETS ? gridDim.x : (unsigned)POSE_SETS;
        unsigned* set_ticket = reinterpret_cast<unsigned*>(acc + q * POSE_SET_FLOATS + (POSE_SET_FLOATS - 1));
        unsigned* ticket = reinterpret_cast<unsigned*>(acc + POSE_SETS * POSE_SET_FLOATS);
        // release / acquire at agent scope on both tickets: this block's additions (ordered before this thread by the
        // barrier above) happen-before the winner's loads of the sets by the memory model, not only by today's codegen
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

}  // namespace sr
