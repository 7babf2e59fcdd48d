// window_joint_bwd.hip — the per-Gaussian pass of splatraster_backward_window_joint: the parameter gradients of a window summed
// over its V views AND the camera gradients of every view, from ONE read of every (view, Gaussian) accumulator row (key-frame poses
// optimised together with the map over a window: splatloc_amd/pose.py WindowPoses).
//
// One thread per Gaussian with a loop over the V views, preprocess_bwd_kernel's mapping: the view-independent work (Sigma3 from
// scale / quaternion, the chain of the summed dL/dSigma3 back to them) is done once per Gaussian, the parameter gradients are
// summed in view order in registers and written once.  Iteration v of the loop also forms the 27 camera partials of row
// (v, i) — dV[4c + r], r < 3; dPM[4c + k], k = 0, 1, 3; the three dcampos terms, zero here: a window has precomputed colours
// only — and reduces them INSIDE the iteration, the way camera_bwd_kernel does for its one view: camera_reduce on view v's slice
// of the workspace.  Every thread of the block takes part in every iteration (V is uniform) and reaches each of its barriers: a
// thread past P or an invisible row contributes zeros.  Nothing waits for another block.
// The arithmetic is projection_bwd.h's, shared with preprocess_bwd_kernel and camera_bwd_kernel; the shell here is this kernel's.
#include "projection_bwd.h"

namespace sr {

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
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P;
    float dmean[3] = {0.f, 0.f, 0.f};
    float dop = 0.f;
    constexpr int NT = TQ > 0 ? 4 * TQ : 1;
    float tsum[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tsum[k] = 0.f;
    [[maybe_unused]] const int ntail = C - (int)GL.SH;
    bool any_visible = false;
    float px = 0.f, py = 0.f, pz = 0.f;
    // 3D covariance and what it was built from — view independent
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // (a thread past P forms S3 below and never reads it)
    float Rm[3][3], sc[3];
    float4 qv;
    if (live) {
        px = means3D[3 * i]; py = means3D[3 * i + 1]; pz = means3D[3 * i + 2];
        sigma3_build(i, mod, scales, rotations, cov3D_precomp, c6, Rm, sc, qv);
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
            projection_row_bwd<true>(W, H, Vm, PM, tanfovx, tanfovy, px, py, pz, S3, mrow, &rec[2 * gr + 1],
                                     dm2x, dm2y, dop, dmean, G3s, pose);
        }
        // the reduction, on the sets and tickets of view v.  Its LDS is reused by the next iteration: three barriers per iteration
        // keep that safe (projection_bwd.h)
        camera_reduce(pose, ws, v, dL_dview, dL_dproj, dL_dcampos);
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
    if (any_visible) sigma3_chain_bwd(cov3D_precomp != nullptr, mod, G3s, Rm, sc, qv, dcov, dscale, drot);
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
