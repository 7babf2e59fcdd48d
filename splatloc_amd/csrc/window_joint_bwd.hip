// window_joint_bwd.hip — the per-Gaussian pass of splatraster_backward_window_joint: the parameter gradients of a window summed
// over its V views AND the camera gradients of every view, from ONE read of every (view, Gaussian) accumulator row (key-frame poses
// optimised together with the map over a window: splatloc_amd/pose.py WindowPoses).
//
// One thread per Gaussian with a loop over the V views, preprocess_bwd_kernel's mapping: the view-independent work (Sigma3 from
// scale / quaternion, the chain of the summed dL/dSigma3 back to them) is done once per Gaussian, the parameter gradients are
// summed in view order in registers and written once.  Iteration v of the loop also forms the 27 camera partials of row
// (v, i) — dV[4c + r], r < 3; dPM[4c + k], k = 0, 1, 3; the three dcampos terms, zero here: a window has precomputed colours
// only — and reduces them INSIDE the iteration, the way camera_bwd_kernel does for its one view: wave_reduce_pack<27>, the four
// waves in LDS, one returning atomic per value and block into set blockIdx.x % POSE_SETS of view v's slice of the workspace, a
// two-level ticket per view; the view's last block sums its sets and writes all 16 + 16 + 3 entries.  Every thread of the block
// takes part in every iteration (V is uniform): a thread past P or an invisible row contributes zeros.  Nothing waits for
// another block.
// The per-row derivative is this file's own copy of preprocess_bwd.hip's (precomputed colours, no RAW chain):
// preprocess_bwd_kernel and camera_bwd_kernel keep their text and their code generation, and the V = 1 results of
// splatraster_backward are what they were.
#include "composite_common.h"

namespace sr {

constexpr int JOINT_WS_FLOATS = (int)(POSE_ACC_BYTES / sizeof(float));   // per view: POSE_SETS sets + the ticket's line (camera_bwd.hip)

// TQ: 16-byte pieces of the per-view row that hold the colour columns behind the shared table (preprocess_bwd.hip)
template <int TQ>
__global__ void __launch_bounds__(256)
window_joint_bwd_kernel(int P, int V, int W, int H, float mod, WinCams cams, WinGrad grads,
                        const float* __restrict__ means3D, const float* __restrict__ scales,
                        const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
                        const float4* __restrict__ rec, const float* __restrict__ gacc, int C, GaccLayout GL, int MO,
                        float* __restrict__ dL_dcolors /*TQ > 0 only*/, float* __restrict__ dL_dmeans3D,
                        float* __restrict__ dL_dopacities, float* __restrict__ dL_dscales,
                        float* __restrict__ dL_drotations, float* __restrict__ dL_dcov3D,
                        float* __restrict__ ws /*V x (zeroed sets + ticket), common.h*/, float* __restrict__ dL_dview,
                        float* __restrict__ dL_dproj, float* __restrict__ dL_dcampos)
{
    __shared__ float s_pose[4][32];
    __shared__ bool s_last;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    float dmean[3] = {0.f, 0.f, 0.f};
    float dop = 0.f;
    constexpr int NT = TQ > 0 ? 4 * TQ : 1;
    float tsum[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tsum[k] = 0.f;
    [[maybe_unused]] const int ntail = C - (int)GL.SH;
    bool any_visible = false;
    float px = 0.f, py = 0.f, pz = 0.f;
    // 3D covariance (recomputed; same formula as the forward) — view independent
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float Rm[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, sc[3] = {0.f, 0.f, 0.f};
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        px = means3D[3 * i]; py = means3D[3 * i + 1]; pz = means3D[3 * i + 2];
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
            c6[0] = L[0][0] * L[0][0] + L[0][1] * L[0][1] + L[0][2] * L[0][2];
            c6[1] = L[0][0] * L[1][0] + L[0][1] * L[1][1] + L[0][2] * L[1][2];
            c6[2] = L[0][0] * L[2][0] + L[0][1] * L[2][1] + L[0][2] * L[2][2];
            c6[3] = L[1][0] * L[1][0] + L[1][1] * L[1][1] + L[1][2] * L[1][2];
            c6[4] = L[1][0] * L[2][0] + L[1][1] * L[2][1] + L[1][2] * L[2][2];
            c6[5] = L[2][0] * L[2][0] + L[2][1] * L[2][1] + L[2][2] * L[2][2];
        }
    }
    const float S3[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float G3s[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // dL/dSigma3 summed over the views

#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        // camera partials of row (v, i): dV[4c + r] (r < 3), dPM[4c + k] (k = 0, 1, 3), dcampos (zero)
        float pose[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) pose[k] = 0.f;
        float dm2x = 0.f, dm2y = 0.f;
        const bool visible = live && cams.radii[v][i] > 0;
        if (visible) {
            any_visible = true;
            const float* __restrict__ view = cams.view[v];
            const float* __restrict__ proj = cams.proj[v];
            const float tanfovx = cams.tanfovx[v], tanfovy = cams.tanfovy[v];
            float Vm[16], PM[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { Vm[k] = view[k]; PM[k] = proj[k]; }
            const size_t gr = (size_t)v * P + i;   // row of (view, Gaussian)
            const float* mrow = gacc + GL.index(gr, (size_t)i, (uint32_t)MO);  // moment record of this row
            if constexpr (TQ > 0) {
                const float4* trow = reinterpret_cast<const float4*>(gacc + GL.index(gr, (size_t)i, GL.SH));
#pragma unroll
                for (int q = 0; q < TQ; ++q) {
                    const float4 t = trow[q];   // (columns behind the tail — moments, padding — are summed along and never written)
                    tsum[4 * q] += t.x; tsum[4 * q + 1] += t.y; tsum[4 * q + 2] += t.z; tsum[4 * q + 3] += t.w;
                }
            }
            const float4 g0 = make_float4(mrow[0], mrow[1], mrow[2], mrow[3]);
            const float4 g1 = make_float4(mrow[4], mrow[5], mrow[6], 0.f);
            const float4 con = rec[2 * gr + 1];  // conic a, b, c, opacity of the forward
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
            // once after the loop
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
            {
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
            {
                const float dh[3] = {dm2x * mw, dm2y * mw, -(mul1 * dm2x + mul2 * dm2y)};  // d/d(hx, hy, hw)
                const float p4[4] = {px, py, pz, 1.f};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                    for (int j = 0; j < 3; ++j) pose[12 + 3 * cc + j] = dh[j] * p4[cc];
            }
        }
        // the reduction of camera_bwd_kernel, on the sets and tickets of view v.  s_pose and s_last are reused by the next
        // iteration: its writes of s_pose come behind this iteration's third barrier, its write of s_last behind two more
        float* __restrict__ acc = ws + (size_t)v * JOINT_WS_FLOATS;
        const float tot = wave_reduce_pack<27>(pose, lane);
        const int slot = (int)(__brev((unsigned)lane) >> 26);
        if (slot < 27) s_pose[wv][slot] = tot;
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
            const unsigned in_set = (gridDim.x - q + (POSE_SETS - 1)) / POSE_SETS;       // blocks that add to set q of this view
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
        // dL/dmeans2D of the view behind its camera sums: the set atomics return into registers, and waiting for them would
        // wait for stores issued in front of them as well (vmcnt counts both)
        if (live) {
            float* __restrict__ dm2 = grads.dL_dmeans2D[v];
            dm2[3 * i] = dm2x;
            dm2[3 * i + 1] = dm2y;
            dm2[3 * i + 2] = 0.f;
        }
    }  // views

    if (!live) return;
    float dscale[3] = {0.f, 0.f, 0.f};
    float drot[4] = {0.f, 0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (any_visible) {
        if (cov3D_precomp) {
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
#pragma unroll
    for (int k = 0; k < 3; ++k) dL_dmeans3D[3 * i + k] = dmean[k];
    if constexpr (TQ > 0) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (k < ntail) dL_dcolors[(size_t)i * C + GL.SH + k] = tsum[k];
    }
    dL_dopacities[i] = dop;
    if (dL_dscales) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dL_dscales[3 * i + k] = dscale[k];
    }
    if (dL_drotations) reinterpret_cast<float4*>(dL_drotations)[i] = make_float4(drot[0], drot[1], drot[2], drot[3]);
    if (dL_dcov3D) {
#pragma unroll
        for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = dcov[k];
    }
}

int launch_window_joint_bwd(const splatraster_settings& s, int32_t P, int32_t V, const WinCams& cams, const WinGrad& grads,
                            const float* means3D, const float* scales, const float* rotations, const float* cov3D_precomp,
                            const float4* rec, const float* gacc, int C, float* dL_dcolors, float* dL_dmeans3D,
                            float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* ws,
                            float* dL_dview, float* dL_dproj, float* dL_dcampos, hipStream_t stream)
{
    if (P <= 0 || V < 1 || V > MAX_VIEWS || !ws || !dL_dview || !dL_dproj || !dL_dcolors || !dL_dmeans3D || !dL_dopacities)
        return SPLATRASTER_ERR_BAD_ARG;
    int st = launch_window_dcolors(P, V, C, gacc, dL_dcolors, stream);    // the shared colour rows / the per-view rows' columns
    if (st) return st;
    const GaccLayout GL = gacc_layout(C, P);
    const int ntail = GL.SH > 0 ? C - (int)GL.SH : 0;   // colour columns of the per-view rows: summed by the kernel below
#define SR_JBWD_ARGS                                                                                                       \
    P, V, s.image_width, s.image_height, s.scale_modifier, cams, grads, means3D, scales, rotations, cov3D_precomp, rec,   \
        gacc, C, GL, gacc_moment_offset(C), dL_dcolors, dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D, \
        ws, dL_dview, dL_dproj, dL_dcampos
    const dim3 grid((unsigned)((P + 255) / 256));
    if (ntail > 4) hipLaunchKernelGGL(window_joint_bwd_kernel<4>, grid, dim3(256), 0, stream, SR_JBWD_ARGS);
    else if (ntail > 0) hipLaunchKernelGGL(window_joint_bwd_kernel<1>, grid, dim3(256), 0, stream, SR_JBWD_ARGS);
    else hipLaunchKernelGGL(window_joint_bwd_kernel<0>, grid, dim3(256), 0, stream, SR_JBWD_ARGS);
#undef SR_JBWD_ARGS
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr
