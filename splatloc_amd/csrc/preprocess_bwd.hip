// preprocess_bwd.hip — per-Gaussian backward of the projection (SURVEY.md §8a
// "PREPROCESS bwd"): conic -> cov2D -> (Sigma3, view-space mean) -> scale / quaternion /
// mean3D, NDC mean2D -> mean3D through the projection, depth -> mean3D, SH -> (sh, mean3D).
//
// One thread per Gaussian; reads the 32-byte record of gradient MOMENTS accumulated by the
// compositing backward, with E = G dL/dalpha and d = mu2D - pixel summed over (pixel, tile):
//   (sum E dx, sum E dy, sum E dx^2, sum E dx dy, sum E dy^2, sum E, sum w g_D, pad)
// turns them into dL/dmean2D (NDC), dL/dconic, dL/dopacity, dL/ddepth with the per-Gaussian
// factors (conic, opacity, 0.5 W, 0.5 H), and chains through the projection.  Plus the forward
// inputs; writes every gradient tensor once.
// HBM-bound: ~100 B read, ~70 B written per Gaussian.
#include "projection_bwd.h"
#include "activation_math.h"

namespace sr {

__constant__ float BSH_C0 = 0.28209479177387814f;
__constant__ float BSH_C1 = 0.4886025119029199f;
__constant__ float BSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                -1.0925484305920792f, 0.5462742152960396f};
__constant__ float BSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                0.3731763325901154f,  -0.4570457994644658f, 1.445305721320277f,
                                -0.5900435899266435f};

__device__ void sh_backward(int deg, int M, const float* sh, float* dsh, const uint8_t* clamped,
                            const float* drgb_in, float ox, float oy, float oz, float* dmean)
{
    const float len = sqrtf(ox * ox + oy * oy + oz * oz);
    const float x = ox / len, y = oy / len, z = oz / len;
    float ddir[3] = {0.f, 0.f, 0.f};
    for (int ch = 0; ch < 3; ++ch) {
        const float d = clamped[ch] ? 0.f : drgb_in[ch];
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#define SHV(k) sh[(k) * 3 + ch]
        dsh[0 * 3 + ch] = BSH_C0 * d;
        if (deg > 0) {
            dsh[1 * 3 + ch] = -BSH_C1 * y * d;
            dsh[2 * 3 + ch] = BSH_C1 * z * d;
            dsh[3 * 3 + ch] = -BSH_C1 * x * d;
            ddx = -BSH_C1 * SHV(3);
            ddy = -BSH_C1 * SHV(1);
            ddz = BSH_C1 * SHV(2);
            if (deg > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                dsh[4 * 3 + ch] = BSH_C2[0] * xy * d;
                dsh[5 * 3 + ch] = BSH_C2[1] * yz * d;
                dsh[6 * 3 + ch] = BSH_C2[2] * (2.f * zz - xx - yy) * d;
                dsh[7 * 3 + ch] = BSH_C2[3] * xz * d;
                dsh[8 * 3 + ch] = BSH_C2[4] * (xx - yy) * d;
                ddx += BSH_C2[0] * y * SHV(4) + BSH_C2[2] * 2.f * -x * SHV(6) + BSH_C2[3] * z * SHV(7) + BSH_C2[4] * 2.f * x * SHV(8);
                ddy += BSH_C2[0] * x * SHV(4) + BSH_C2[1] * z * SHV(5) + BSH_C2[2] * 2.f * -y * SHV(6) + BSH_C2[4] * 2.f * -y * SHV(8);
                ddz += BSH_C2[1] * y * SHV(5) + BSH_C2[2] * 4.f * z * SHV(6) + BSH_C2[3] * x * SHV(7);
                if (deg > 2) {
                    dsh[9 * 3 + ch] = BSH_C3[0] * y * (3.f * xx - yy) * d;
                    dsh[10 * 3 + ch] = BSH_C3[1] * xy * z * d;
                    dsh[11 * 3 + ch] = BSH_C3[2] * y * (4.f * zz - xx - yy) * d;
                    dsh[12 * 3 + ch] = BSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * d;
                    dsh[13 * 3 + ch] = BSH_C3[4] * x * (4.f * zz - xx - yy) * d;
                    dsh[14 * 3 + ch] = BSH_C3[5] * z * (xx - yy) * d;
                    dsh[15 * 3 + ch] = BSH_C3[6] * x * (xx - 3.f * yy) * d;
                    ddx += BSH_C3[0] * SHV(9) * 6.f * xy + BSH_C3[1] * SHV(10) * yz + BSH_C3[2] * SHV(11) * -2.f * xy +
                           BSH_C3[3] * SHV(12) * -6.f * xz + BSH_C3[4] * SHV(13) * (-3.f * xx + 4.f * zz - yy) +
                           BSH_C3[5] * SHV(14) * 2.f * xz + BSH_C3[6] * SHV(15) * 3.f * (xx - yy);
                    ddy += BSH_C3[0] * SHV(9) * 3.f * (xx - yy) + BSH_C3[1] * SHV(10) * xz +
                           BSH_C3[2] * SHV(11) * (-3.f * yy + 4.f * zz - xx) + BSH_C3[3] * SHV(12) * -6.f * yz +
                           BSH_C3[4] * SHV(13) * -2.f * xy + BSH_C3[5] * SHV(14) * -2.f * yz +
                           BSH_C3[6] * SHV(15) * -6.f * xy;
                    ddz += BSH_C3[1] * SHV(10) * xy + BSH_C3[2] * SHV(11) * 8.f * yz +
                           BSH_C3[3] * SHV(12) * 3.f * (2.f * zz - xx - yy) + BSH_C3[4] * SHV(13) * 8.f * xz +
                           BSH_C3[5] * SHV(14) * (xx - yy);
                }
            }
        }
#undef SHV
        for (int k = (deg + 1) * (deg + 1); k < M; ++k) dsh[k * 3 + ch] = 0.f;
        ddir[0] += ddx * d;
        ddir[1] += ddy * d;
        ddir[2] += ddz * d;
    }
    const float dot = x * ddir[0] + y * ddir[1] + z * ddir[2];
    dmean[0] += (ddir[0] - x * dot) / len;
    dmean[1] += (ddir[1] - y * dot) / len;
    dmean[2] += (ddir[2] - z * dot) / len;
}

// One thread per Gaussian, looping over the V views of the window: the contributions of every view (accumulator
// row g = v * P + i, forward record rec[g], the view's camera) are summed in view order into ONE set of parameter
// gradients, written once — no per-view gradient tensors, no accumulation kernels, a deterministic sum.
// dL/dmeans2D stays per view (GaussianModel.add_densification_stats reads it per view).
// TQ > 0 (C >= 32 with C % 16 != 0; GaccLayout, common.h): the colour columns that are not in the shared table lie in front of the
// moments in the per-view row this kernel reads anyway — they are summed here, in view order, and written to dL_dcolors[i][SH ..]
// (copy_shared_dcolors_kernel copies the shared columns).  TQ = 16-byte pieces of the row that hold them (the row is 64-byte
// aligned): 1 for the headline's three tail channels (C = 35, 36), 4 for any longer tail.
template <bool POSE, bool RAW = false, int TQ = 0>
__global__ void __launch_bounds__(256)
preprocess_bwd_kernel(int P, int V, int W, int H, float mod, int sh_degree, int M, WinCams cams, WinGrad grads,
                      const float* __restrict__ means3D, const float* __restrict__ shs,
                      const float* __restrict__ scales, const float* __restrict__ rotations,
                      const float* __restrict__ cov3D_precomp,
                      const uint8_t* __restrict__ clamped,
                      const float4* __restrict__ rec, const float* __restrict__ gacc, int C, GaccLayout GL, int MO,
                      float* __restrict__ dL_dcolors /*TQ > 0 only*/, float* __restrict__ dL_dmeans3D,
                      float* __restrict__ dL_dopacities, float* __restrict__ dL_dscales,
                      float* __restrict__ dL_drotations, float* __restrict__ dL_dcov3D,
                      float* __restrict__ dL_dshs, float* __restrict__ dL_dview, float* __restrict__ dL_dproj,
                      float* __restrict__ dL_dcampos, float* __restrict__ pose_acc /*POSE: zeroed sets + ticket (common.h)*/,
                      RawBwd raw /*RAW: the raw parameters and their gradient outputs (common.h)*/)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // pose partials of this Gaussian: dV[4c + r] (r < 3), dPM[4c + k] (k = 0, 1, 3), dcampos   (V == 1 only)
    float pose[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) pose[k] = 0.f;
    float dmean[3] = {0.f, 0.f, 0.f};
    float dscale[3] = {0.f, 0.f, 0.f};
    float drot[4] = {0.f, 0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dop = 0.f;
    float csum[4] = {0.f, 0.f, 0.f, 0.f};   // RAW: dL/dcolours of this Gaussian (a view that does not see it left its row at +0: skipping it is exact)
    constexpr int NT = TQ > 0 ? 4 * TQ : 1;    // TQ > 0: the same for the colour columns of the per-view row
    float tsum[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tsum[k] = 0.f;
    [[maybe_unused]] const int ntail = C - (int)GL.SH;
    if (i < P) {
    bool any_visible = false;
    const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
    // 3D covariance and what it was built from — view independent
    float c6[6], Rm[3][3], sc[3];
    float4 qv;
    sigma3_build(i, mod, scales, rotations, cov3D_precomp, c6, Rm, sc, qv);
    const float S3[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float G3s[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // dL/dSigma3 summed over the views

#pragma unroll 1
    for (int v = 0; v < V; ++v) {
    const float* __restrict__ view = cams.view[v];
    const float* __restrict__ proj = cams.proj[v];
    const float* __restrict__ campos_p = cams.campos[v];
    const float tanfovx = cams.tanfovx[v], tanfovy = cams.tanfovy[v];
    float Vm[16], PM[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { Vm[k] = view[k]; PM[k] = proj[k]; }
    const size_t gr = (size_t)v * P + i;   // row of (view, Gaussian)
    float dm2x = 0.f, dm2y = 0.f;
    const bool visible = cams.radii[v][i] > 0;
    if (visible) {
        any_visible = true;
        const float* mrow = gacc + GL.index(gr, (size_t)i, (uint32_t)MO);  // moment record of this row
        if constexpr (RAW) {    // the row's colour columns (C <= 4: the moments' own 64-byte line), summed in view order like gather_dcolors_kernel
            const float4 cr = *reinterpret_cast<const float4*>(gacc + GL.index(gr, (size_t)i, 0u));
            csum[0] += cr.x; csum[1] += cr.y; csum[2] += cr.z; csum[3] += cr.w;
        }
        if constexpr (TQ > 0) {
            const float4* trow = reinterpret_cast<const float4*>(gacc + GL.index(gr, (size_t)i, GL.SH));
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
                const float4 t = trow[q];   // (columns behind the tail — moments, padding — are summed along and never written)
                tsum[4 * q] += t.x; tsum[4 * q + 1] += t.y; tsum[4 * q + 2] += t.z; tsum[4 * q + 3] += t.w;
            }
        }
        projection_row_bwd<POSE>(W, H, Vm, PM, tanfovx, tanfovy, px, py, pz, S3, mrow, &rec[2 * gr + 1],
                                 dm2x, dm2y, dop, dmean, G3s, pose);
        if (shs) {   // single-view calls only
            // the direction's term on its own, then joined to dmean (the same sum as adding it in place: 0 + term is exact).  Taken
            // back out of dmean as (dmean - before), it came with the rounding of the projection's part, often tens of times larger
            float dsh_mean[3] = {0.f, 0.f, 0.f};
            sh_backward(sh_degree, M, shs + (size_t)i * 3 * M, dL_dshs + (size_t)i * 3 * M, clamped + 3 * (size_t)i,
                        gacc + GL.index(gr, (size_t)i, 0u), px - campos_p[0], py - campos_p[1], pz - campos_p[2], dsh_mean);
            dmean[0] += dsh_mean[0];
            dmean[1] += dsh_mean[1];
            dmean[2] += dsh_mean[2];
            if (POSE) {  // direction = normalize(p - campos)
                pose[24] = -dsh_mean[0];
                pose[25] = -dsh_mean[1];
                pose[26] = -dsh_mean[2];
            }
        }
    } else if (shs && dL_dshs) {
        for (int k = 0; k < 3 * M; ++k) dL_dshs[(size_t)i * 3 * M + k] = 0.f;
    }
    float* __restrict__ dm2 = grads.dL_dmeans2D[v];
    dm2[3 * i] = dm2x;
    dm2[3 * i + 1] = dm2y;
    dm2[3 * i + 2] = 0.f;
    }  // views

    if (any_visible) sigma3_chain_bwd(cov3D_precomp != nullptr, mod, G3s, Rm, sc, qv, dcov, dscale, drot);
    }  // i < P
    if (POSE) camera_reduce(pose, pose_acc, 0, dL_dview, dL_dproj, dL_dcampos);
    // the per-Gaussian gradients are written AFTER the camera sums went out: the set atomics return into registers and nothing
    // but loads precedes them — behind the stores below, waiting for them would wait for the stores as well (vmcnt counts both)
    if (i < P) {
#pragma unroll
    for (int k = 0; k < 3; ++k) dL_dmeans3D[3 * i + k] = dmean[k];
    if constexpr (TQ > 0) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (k < ntail) dL_dcolors[(size_t)i * C + GL.SH + k] = tsum[k];
    }
    if constexpr (RAW) {
        // the chain through the activations, with activations.hip's own arithmetic (activation_math.h): bit-identical to
        // gather_dcolors_kernel + activate_bwd_kernel behind the plain kernel
        if (raw.reg_row_grad) {     // torch's `d_sca + ((w * out[1]) * row_grad)`: three separately rounded operations (activation_math.h)
            const float o1 = raw.reg_out[1], rg = raw.reg_row_grad[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) dscale[k] = act_add_scaled(dscale[k], raw.reg_weight, o1, rg);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) raw.d_scaling[3 * i + k] = dscale[k] * expf(raw.scaling[3 * (size_t)i + k]);
        reinterpret_cast<float4*>(raw.d_rotation)[i] =
            act_normalize_bwd(reinterpret_cast<const float4*>(raw.rotation)[i], make_float4(drot[0], drot[1], drot[2], drot[3]));
        raw.d_opacity[i] = act_sigmoid_bwd(dop, raw.opacity[i]);
        // dL/dcolours (csum: summed in the view loop), then d cat / d clamp_min / d eval_sh (degree 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = act_rgb_raw_deg0(raw.f_dc[3 * (size_t)i + c]) >= 0.0f ? csum[c] : 0.0f;
            raw.d_f_dc[3 * (size_t)i + c] = ACT_SH_C0 * g;
        }
        if (raw.E) raw.d_extra[i] = csum[3];
        return;
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
}

// dL/dcolors [P, C] out of the 64-byte aligned accumulator rows: one thread per element,
// contiguous reads inside a row, fully coalesced writes.
// deterministic debug mode: the fixed-point accumulator rows -> the float rows the kernels below read
// (dst holds, per element, the bit pattern of the largest |partial| that went into src — composite_bwd.hip acc_add:
//  the fixed point of the element is 2^-(170 - headroom_drop - its biased exponent); the same expression is evaluated here)
__global__ void __launch_bounds__(256)
fixed_to_float_kernel(int64_t n, const long long* __restrict__ src, float* __restrict__ dst, int headroom_drop)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned mb = reinterpret_cast<const unsigned*>(dst)[e];
    const int eb = (int)((mb >> 23) & 0xffu);
    if (eb == 255) {   // a non-finite partial (composite_bwd.hip acc_add): NaN, or the infinity whose sign(s) were counted
        const unsigned long long cnt = (unsigned long long)src[e];
        const bool pos = (cnt & 0xffffffffull) != 0, neg = (cnt >> 32) != 0;
        dst[e] = ((mb & 0x7fffffu) || pos == neg) ? __builtin_nanf("") : (neg ? -__builtin_inff() : __builtin_inff());
        return;
    }
    dst[e] = (float)ldexp((double)src[e], -(170 - headroom_drop - (eb > 0 ? eb : 1)));
}

int launch_fixed_to_float(int64_t n, const long long* src, float* dst, int headroom_drop, hipStream_t stream)
{
    if (n <= 0) return SPLATRASTER_OK;
    hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, src, dst, headroom_drop);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

// C < 32 (SH = 0): the colour columns of the V per-view rows of every Gaussian, summed in view order.
__global__ void __launch_bounds__(256)
gather_dcolors_kernel(int64_t n, int C, GaccLayout GL, int V, const float* __restrict__ gacc,
                      float* __restrict__ dL_dcolors)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int64_t i = e / C;
    const int ch = (int)(e - i * C);
    float sum = gacc[GL.index((size_t)i, (size_t)i, (uint32_t)ch)];
    for (int v = 1; v < V; ++v) sum += gacc[GL.index((size_t)v * GL.P + (size_t)i, (size_t)i, (uint32_t)ch)];   // the feature table is shared by the views
    dL_dcolors[e] = sum;
}
// C >= 32: the views already added into ONE row per Gaussian (the atomics formed the sum over the views): a coalesced copy
// [P][SH] -> dL_dcolors[:, :SH], no view loop; the columns SH .. C - 1 are preprocess_bwd_kernel<.., TQ>'s
__global__ void __launch_bounds__(256)
copy_shared_dcolors_kernel(int64_t n /*P * SH*/, int C, GaccLayout GL, const float* __restrict__ gacc, float* __restrict__ dL_dcolors)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int64_t i = e / GL.SH;
    const uint32_t ch = (uint32_t)(e - i * GL.SH);
    dL_dcolors[i * C + ch] = gacc[GL.index((size_t)i, (size_t)i, ch)];
}

// dL_dcolors [P, C] of precomputed colours out of the accumulator rows: the copy of the shared table (C >= 32; its tail columns
// are the per-Gaussian kernel's) or the gather over the V per-view rows
int launch_window_dcolors(int32_t P, int32_t V, int C, const float* gacc, float* dL_dcolors, hipStream_t stream)
{
    const GaccLayout GL = gacc_layout(C, P);
    const int64_t n = (int64_t)P * (GL.SH ? (int)GL.SH : C);
    if (GL.SH)
        hipLaunchKernelGGL(copy_shared_dcolors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, GL, gacc,
                           dL_dcolors);
    else
        hipLaunchKernelGGL(gather_dcolors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, GL, V, gacc,
                           dL_dcolors);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int launch_preprocess_bwd(const splatraster_settings& s, int32_t P, int32_t V, const WinCams& cams, const WinGrad& grads,
                          const float* means3D, const float* shs, const float* scales, const float* rotations,
                          const float* cov3D_precomp, const uint8_t* clamped, const float4* rec, const float* gacc, int C,
                          float* dL_dcolors, float* dL_dmeans3D, float* dL_dopacities, float* dL_dscales,
                          float* dL_drotations, float* dL_dcov3D, float* dL_dshs, float* dL_dview,
                          float* dL_dproj, float* dL_dcampos, float* pose_acc, hipStream_t stream, const RawBwd* raw)
{
    if (P == 0) return SPLATRASTER_OK;
    const GaccLayout GL = gacc_layout(C, P);
    const int ntail = (dL_dcolors && !raw && GL.SH > 0) ? C - (int)GL.SH : 0;   // colour columns of the per-view rows: summed by the kernel below
    if (dL_dcolors && !raw) {
        const int st = launch_window_dcolors(P, V, C, gacc, dL_dcolors, stream);
        if (st) return st;
    }
    const bool pose = dL_dview && dL_dproj;      // (the accumulator sets behind gacc were zeroed with the rows: capi.hip)
    if (pose && !pose_acc) return SPLATRASTER_ERR_BAD_ARG;
#define SR_PBWD_ARGS                                                                                              \
    P, V, s.image_width, s.image_height, s.scale_modifier, s.sh_degree, s.sh_coeffs, cams, grads, means3D,         \
        shs, scales, rotations, cov3D_precomp, clamped, rec, gacc, C, GL,                                          \
        gacc_moment_offset(C), dL_dcolors, dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations,                              \
        dL_dcov3D, dL_dshs, dL_dview, dL_dproj, dL_dcampos, pose_acc, (raw ? *raw : RawBwd{})
    if (raw) {
        if (pose || shs || cov3D_precomp || !scales || !rotations || raw->E > 1) return SPLATRASTER_ERR_UNSUPPORTED;   // (C <= 4: the colour columns share the moments' line)
        hipLaunchKernelGGL((preprocess_bwd_kernel<false, true>), dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
    } else if (pose) {
        if (ntail > 4) hipLaunchKernelGGL((preprocess_bwd_kernel<true, false, 4>), dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
        else if (ntail > 0) hipLaunchKernelGGL((preprocess_bwd_kernel<true, false, 1>), dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
        else hipLaunchKernelGGL(preprocess_bwd_kernel<true>, dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
    } else {
        if (ntail > 4) hipLaunchKernelGGL((preprocess_bwd_kernel<false, false, 4>), dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
        else if (ntail > 0) hipLaunchKernelGGL((preprocess_bwd_kernel<false, false, 1>), dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
        else hipLaunchKernelGGL(preprocess_bwd_kernel<false>, dim3((P + 255) / 256), dim3(256), 0, stream, SR_PBWD_ARGS);
    }
#undef SR_PBWD_ARGS
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr
