// camera_bwd.hip — the camera gradients of the V views of a window, and nothing else (splatraster_backward_window_cameras:
// pose refinement of a window of query frames against a frozen map, splatloc_amd/pose.py refine_poses).
//
// One thread per (view, Gaussian), grid (ceil(P / 256), V): a block never straddles two views.  A thread reads what
// preprocess_bwd_kernel<true> reads of that row — the forward's record, the moments the compositing backward left in the view's
// accumulator row, the view's camera — and forms the same 27 partials with the same code (projection_bwd.h: dV[4c + r], r < 3;
// dPM[4c + k], k = 0, 1, 3; the three dcampos terms, zero here: a window has precomputed colours only).  No per-Gaussian
// gradient, no dL/dmeans2D is stored: the row's parameter terms go into locals nobody reads, the compiler drops them and the
// loads that only feed them, and the kernel writes 35 floats per view.
// The reduction is camera_reduce on the sets and tickets of the block's OWN view.
#include "projection_bwd.h"

namespace sr {

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
        float c6[6], Rm[3][3], sc[3];
        float4 qv;
        sigma3_build(i, mod, scales, rotations, cov3D_precomp, c6, Rm, sc, qv);
        const float S3[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
        const size_t gr = (size_t)v * P + i;   // row of (view, Gaussian)
        const float* mrow = gacc + GL.index(gr, (size_t)i, (uint32_t)MO);  // moment record of this row
        // the parameter terms of the row: not wanted here
        float dm2x, dm2y, dop = 0.f, dmean[3] = {0.f, 0.f, 0.f}, G3s[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        projection_row_bwd<true>(W, H, Vm, PM, tanfovx, tanfovy, px, py, pz, S3, mrow, &rec[2 * gr + 1],
                                 dm2x, dm2y, dop, dmean, G3s, pose);
    }
    camera_reduce(pose, ws, v, dL_dview, dL_dproj, dL_dcampos);
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
