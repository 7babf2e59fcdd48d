// losses.hip — SplatLoc's per-view mapping loss and its gradient w.r.t. the rendered buffers in
// ONE pass over the pixels.  Replaces the chain of elementwise torch kernels
// (masks, exposure affine, abs, three means, sigmoid, BCE) and the equally long autograd chain of
//   utils/utils.py:55-82     get_loss_mapping / get_loss_mapping_rgbd
//   train_gaussians.py:38-42 get_loss_marker
// as summed per view at train_gaussians.py:217-218:
//   loss = mean |m_rgb x - m_rgb gt| + mean |m_d depth - m_d gt_depth| + mean BCE(sigmoid(marker), kp)
//   x = exp(a) image + b,  m_rgb = sum_c gt[c] > threshold,  m_d = gt_depth > 0.01
// kp is the float score map used as a SOFT BCE target (gt.view(-1).float(), train_gaussians.py:40).
// HBM-bound: reads 9 planes, writes 5 planes per pixel.  The five sums (three loss
// terms, dL/da, dL/db) are reduced per block in double and finished by a one-block kernel:
// deterministic, no atomics.
#include "common.h"
#include "reduce.h"

namespace sr {

constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_SUMS = 5;  // l1 rgb, l1 depth, bce, d/da, d/db

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// the views of a window in ONE launch pair (blockIdx.y = view): every view's blocks, partial sums and their order are those
// of the single-view launch, so the window's per-view results are bit-identical to V separate calls
struct LossViews {
    const float* image[MAX_VIEWS]; const float* depth[MAX_VIEWS]; const float* marker[MAX_VIEWS];
    const float* gt_image[MAX_VIEWS]; const float* gt_depth[MAX_VIEWS]; const float* kp[MAX_VIEWS];
    const float* exposure[MAX_VIEWS];   // [2] = a, b or NULL
    float* g_image[MAX_VIEWS]; float* g_depth[MAX_VIEWS]; float* g_marker[MAX_VIEWS];
};

__global__ void __launch_bounds__(LOSS_BLOCK)
mapping_loss_kernel(int HW, LossViews lv, float threshold, double* __restrict__ partial_all /*[V][gridDim.x][LOSS_SUMS]*/)
{
    const int view = blockIdx.y;
    const float* __restrict__ image = lv.image[view];
    const float* __restrict__ depth = lv.depth[view];
    const float* __restrict__ marker = lv.marker[view];
    const float* __restrict__ gt_image = lv.gt_image[view];
    const float* __restrict__ gt_depth = lv.gt_depth[view];
    const float* __restrict__ kp = lv.kp[view];
    const float* __restrict__ exposure = lv.exposure[view];
    float* __restrict__ g_image = lv.g_image[view];
    float* __restrict__ g_depth = lv.g_depth[view];
    float* __restrict__ g_marker = lv.g_marker[view];
    double* __restrict__ partial = partial_all + (size_t)view * gridDim.x * LOSS_SUMS;
    const float ea = exposure ? expf(exposure[0]) : 1.0f;
    const float eb = exposure ? exposure[1] : 0.0f;
    const float inv_rgb = 1.0f / (3.0f * (float)HW), inv_n = 1.0f / (float)HW;
    double acc[LOSS_SUMS] = {0, 0, 0, 0, 0};
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const float t0 = gt_image[p], t1 = gt_image[HW + p], t2 = gt_image[2 * HW + p];
        const float m = ((t0 + t1) + t2) > threshold ? 1.0f : 0.0f;
        const float gt[3] = {t0, t1, t2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = image[c * HW + p];
            const float x = exposure ? ea * v + eb : v;
            const float diff = x * m - gt[c] * m;
            const float gx = sgn(diff) * m * inv_rgb;
            acc[0] += fabsf(diff);
            acc[3] += (double)(gx * v);
            acc[4] += (double)gx;
            g_image[c * HW + p] = gx * ea;
        }
        const float gd = gt_depth[p];
        const float md = gd > 0.01f ? 1.0f : 0.0f;
        const float dd = depth[p] * md - gd * md;
        acc[1] += fabsf(dd);
        g_depth[p] = sgn(dd) * md * inv_n;
        const float s = 1.0f / (1.0f + expf(-marker[p]));
        const float y = kp[p];   // soft target: the raw key-point score map (utils/dataset.py:94, camera_utils.py:75)
        // the logarithms reach 8 and more, where one float32 ulp of logf is 5e-7 of a term: over a small frame that is more
        // than an ulp of the mean.  s and 1 - s stay the reference's float32 values (at a logit of 17 s is 1 and the clamp acts)
        const double lp = fmax(log((double)s), -100.0), lq = fmax(log((double)(1.0f - s)), -100.0);
        acc[2] -= (double)y * lp + (1.0 - (double)y) * lq;
        const float sq = s * (1.0f - s);
        g_marker[p] = (s - y) / fmaxf(sq, 1e-12f) * sq * inv_n;
    }
    __shared__ double s_red[LOSS_BLOCK / WAVE][LOSS_SUMS];
    block_sum<LOSS_BLOCK>(acc, s_red);
    if (threadIdx.x < LOSS_SUMS) partial[(size_t)blockIdx.x * LOSS_SUMS + threadIdx.x] = block_total(s_red, threadIdx.x);
}

__global__ void __launch_bounds__(LOSS_BLOCK)
mapping_loss_finish_kernel(int blocks, int HW, const double* __restrict__ partial_all, LossViews lv,
                           float* __restrict__ out_all /*[V][4]*/)
{
    const int view = blockIdx.x;
    const double* __restrict__ partial = partial_all + (size_t)view * blocks * LOSS_SUMS;
    const float* __restrict__ exposure = lv.exposure[view];
    float* __restrict__ out = out_all + 4 * view;
    __shared__ double s_red[LOSS_BLOCK / WAVE][LOSS_SUMS];
    double t[LOSS_SUMS];
    partials_block_sum<LOSS_BLOCK>(blocks, partial, s_red, t);
    if (threadIdx.x == 0) {
        const double n = (double)HW;
        out[0] = (float)(t[0] / (3.0 * n) + t[1] / n);                 // get_loss_mapping
        out[1] = (float)(t[2] / n);                                    // get_loss_marker
        out[2] = exposure ? (float)(t[3] * (double)expf(exposure[0])) : 0.0f;  // dL/d exposure_a
        out[3] = exposure ? (float)t[4] : 0.0f;                        // dL/d exposure_b
    }
}

static int loss_blocks(int32_t HW)
{
    int blocks = (HW + LOSS_BLOCK - 1) / LOSS_BLOCK;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return blocks;
}

static size_t mapping_loss_workspace_bytes(int32_t HW) { return (size_t)loss_blocks(HW) * LOSS_SUMS * sizeof(double); }

// V views (host array of per-view pointers), out [V][4], workspace V x mapping_loss_workspace_bytes(HW)
static int launch_mapping_loss_window(int32_t V, int32_t HW, const splatraster_loss_view* views, float threshold, float* out,
                               void* workspace, hipStream_t stream)
{
    LossViews lv{};
    for (int v = 0; v < V; ++v) {
        lv.image[v] = views[v].image; lv.depth[v] = views[v].depth; lv.marker[v] = views[v].marker;
        lv.gt_image[v] = views[v].gt_image; lv.gt_depth[v] = views[v].gt_depth; lv.kp[v] = views[v].kp;
        lv.exposure[v] = views[v].exposure;
        lv.g_image[v] = views[v].g_image; lv.g_depth[v] = views[v].g_depth; lv.g_marker[v] = views[v].g_marker;
    }
    const int blocks = loss_blocks(HW);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(mapping_loss_kernel, dim3(blocks, V), dim3(LOSS_BLOCK), 0, stream, HW, lv, threshold, partial);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(mapping_loss_finish_kernel, dim3(V), dim3(LOSS_BLOCK), 0, stream, blocks, HW, partial, lv, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

static int launch_mapping_loss(int32_t HW, const float* image, const float* depth, const float* marker,
                        const float* gt_image, const float* gt_depth, const float* kp, float threshold,
                        const float* exposure, float* g_image, float* g_depth, float* g_marker, float* out,
                        void* workspace, hipStream_t stream)
{
    const splatraster_loss_view one{image, depth, marker, gt_image, gt_depth, kp, exposure, g_image, g_depth, g_marker};
    return launch_mapping_loss_window(1, HW, &one, threshold, out, workspace, stream);
}


// ---------------------------------------------------------------------------------------------
// Colour-refinement loss (train_gaussians.py:283-285):
//     loss = (1 - lambda) l1_loss(image, gt) + lambda (1 - ssim(image, gt))
// l1_loss / ssim: gaussian_splatting/utils/loss_utils.py:21-22, 42-102 (11x11 Gaussian window,
// sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements).
// The reference runs 5 dense 11x11 grouped convolutions forward and their autograd backward;
// here the window is applied separably out of LDS, in two kernels:
//   refine_fwd: per 32x16 tile (+5 halo) the blurred first and second moments of x and y (about a per-tile shift: SHIFTED
//               MOMENTS below) -> SSIM map value and its partials dm/dmu1, dm/ds1, dm/ds12 (s1 = blur(x^2),
//               s12 = blur(xy)); tile sums of m and |x - y|
//   refine_bwd: dL/dx = (1-lambda) sign(x-y)/n - lambda/n (blur(dm/dmu1) + 2 x blur(dm/ds1) + y blur(dm/ds12))
// (the window is symmetric, so the adjoint of the zero-padded convolution is the same blur).
// ---------------------------------------------------------------------------------------------
constexpr int RT = 16;            // tile edge of eval_metrics_kernel
constexpr int RH = 5;             // window radius
constexpr int RW = 2 * RH + 1;    // 11 taps

struct RefineWindow { float w[RW]; double mass; /* sum w in double: the float32 window does not sum to 1 */ };

// SHIFTED MOMENTS.  sigma = E[x^2] - mu^2 cancels in float32: over a smooth bright region both terms are ~0.6 and their
// rounding, ~3e-8, stands against C2 = 9e-4 — 1e-4 of every pixel's SSIM, and that is the regime the refinement loop
// converges into.  A variance does not depend on a shift, so the SSIM kernels blur the moments of d = x - c and
// e = y - c: their loader functors subtract c, one value per tile, the median of three gt samples of the tile (one bright pixel on
// a dark ground leaves c dark).  Zero padding stays exact: a pixel outside the image contributes 0 to the shifted sums,
// and with S = the window mass inside the image and U = 1 - S
//     mu    = E0[d] + c S
//     sigma = E0[d^2] - E0[d]^2 + c U (2 E0[d] + c S)            (sigma12: E0[d e] - E0[d] E0[e] + c U (E0[d] + E0[e] + c S))
// S, U and these few terms are formed in double and rounded once: at an image border U is most of the window and the terms
// are as large as the unshifted ones.  Inside, U = 1 - mass^2 = 9e-8.  Where c = 0 these are the unshifted forms.
// For finite inputs only: a NaN or an infinity among the three samples reaches every statistic of its tile (inf - inf), where
// the unshifted sums carried it no further than the windows that touch it.  Images and ground truth are finite by contract.
__device__ __forceinline__ float tile_shift(const float* __restrict__ gt_plane, int H, int W, int y0, int x0, int th, int tw)
{
    const float a = gt_plane[(size_t)min(y0 + th / 4, H - 1) * W + min(x0 + tw / 4, W - 1)];
    const float b = gt_plane[(size_t)min(y0 + th / 2, H - 1) * W + min(x0 + tw / 2, W - 1)];
    const float c = gt_plane[(size_t)min(y0 + 3 * th / 4, H - 1) * W + min(x0 + 3 * tw / 4, W - 1)];
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));   // the median
}

__device__ __forceinline__ double window_cover(const RefineWindow& win, int g, int n)
{
    if (g >= RH && g + RH < n) return win.mass;
    double inside = 0.0;
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const int gk = g + k - RH;
        if (gk >= 0 && gk < n) inside += (double)win.w[k];
    }
    return inside;
}

struct SsimStats { float mu1, mu2, sig1, sig2, sig12; };
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

// S: the window mass inside the image at the output (gy, gx)
__device__ __forceinline__ double ssim_cover(const RefineWindow& win, int gy, int gx, int H, int W)
{
    return window_cover(win, gx, W) * window_cover(win, gy, H);
}

// v = E0[d], E0[e], E0[d^2], E0[e^2], E0[d e] of an output whose window has the mass S inside the image
__device__ __forceinline__ SsimStats ssim_stats(const float v[5], float c, double S)
{
    const double U = 1.0 - S;
    const double cs = (double)c * S, cu = (double)c * U;
    const double d = (double)v[0], e = (double)v[1];
    SsimStats t;
    t.mu1 = (float)(d + cs);
    t.mu2 = (float)(e + cs);
    t.sig1 = (float)(((double)v[2] - d * d) + cu * (d + d + cs));
    t.sig2 = (float)(((double)v[3] - e * e) + cu * (e + e + cs));
    t.sig12 = (float)(((double)v[4] - d * e) + cu * (d + e + cs));
    return t;
}

// Round 5: the two refinement kernels work on 32x16 tiles with REGISTER-BLOCKED passes — a horizontal work item loads 14
// consecutive taps once and produces 4 adjacent outputs, a vertical one loads 12 rows and produces 2 (the 16x16 / one-output-per-thread form
// read LDS 22 + 55 times per output): refine_fwd 22.1 -> 18.4 us, refine_bwd 16.1 -> 14.4 us (profiles/r05_ab_probes.txt #8;
// what was left then was the load -> barrier -> pass -> barrier -> pass -> store chain, not arithmetic).  Every output is
// accumulated tap by tap in ascending order.
// The shifted moments and the double-precision statistics and partials that followed (about 60 FP64 operations and one FP64
// division per output, for the edge suite's 4 x E_ref bounds) are arithmetic the forward did not have, and they cost: at
// 3x1080x1920 on an MI355X (kernel trace, mean of 1530 launches) refine_fwd 76.5 -> 94.0 us, eval_metrics_kernel
// 111.0 -> 123.7 us, refine_bwd unchanged at 62.8 us; the maps and the gradient are no longer bit-identical to Round 5's.
constexpr int FW = 32, FH = 16;               // tile of the refinement kernels

// THE SEPARABLE BLUR OUT OF LDS, written once for the three kernels below: a TW x TH tile and its halo of RH are loaded as QI
// planes, blurred along the rows into Q planes (HO adjacent outputs per work item) and along the columns into the tile's
// outputs (VO per thread); a barrier stands between the steps, in the kernel.  Every output is accumulated tap by tap in
// ascending order as  wk * plane, so a tile shape and a blocking decide who computes a blurred value, never its bits (what
// the SSIM kernels blur does depend on the tile: tile_shift takes its three samples at fractions of the tile's edges).
//   refine_fwd, refine_bwd: 32x16, HO = 4, VO = 2 (5 and 3 planes);   eval_metrics: 16x16, HO = VO = 1 (5 planes).
// Loader: pixel(o, own, v) is called for every element of tile + halo INSIDE the image (o = gy W + gx, own = one of the tile's
// own pixels) and fills the QI values LDS is to hold; outside the image LDS holds 0 (zero padding).  What a kernel does to a
// pixel on the way in (the shift, eval's clamp) and the sums it takes over its own pixels live in that functor.
template <int TW, int TH, int THREADS, int QI, class Pixel>
__device__ __forceinline__ void blur_load_tile(float (&s_in)[QI][TH + 2 * RH][TW + 2 * RH + 1], int H, int W, int y0, int x0,
                                               Pixel&& pixel)
{
    constexpr int EW = TW + 2 * RH, EH = TH + 2 * RH;
    for (int e = threadIdx.x; e < EH * EW; e += THREADS) {
        const int r = e / EW, c = e - r * EW;
        const int gy = y0 + r - RH, gx = x0 + c - RH;
        float v[QI];
#pragma unroll
        for (int q = 0; q < QI; ++q) v[q] = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) pixel((size_t)gy * W + gx, r >= RH && r < RH + TH && c >= RH && c < RH + TW, v);
#pragma unroll
        for (int q = 0; q < QI; ++q) s_in[q][r][c] = v[q];
    }
}

// rows: MOMENTS blurs x, y, x^2, y^2, x y of the two planes loaded (Q = 5), else the QI planes as they are
template <int TW, int TH, int THREADS, int HO, bool MOMENTS, int QI, int Q>
__device__ __forceinline__ void blur_rows(const RefineWindow& win, const float (&s_in)[QI][TH + 2 * RH][TW + 2 * RH + 1],
                                          float (&s_h)[Q][TH + 2 * RH][TW + 1])
{
    static_assert(MOMENTS ? (QI == 2 && Q == 5) : Q == QI, "planes");
    constexpr int G = TW / HO, NT = RW + HO - 1;   // work items per row; taps an item loads
    for (int e = threadIdx.x; e < (TH + 2 * RH) * G; e += THREADS) {
        const int r = e / G, c0 = (e - r * G) * HO;
        float p[Q][NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
#pragma unroll
            for (int q = 0; q < QI; ++q) p[q][k] = s_in[q][r][c0 + k];
            if constexpr (MOMENTS) {
                p[2][k] = p[0][k] * p[0][k];
                p[3][k] = p[1][k] * p[1][k];
                p[4][k] = p[0][k] * p[1][k];
            }
        }
#pragma unroll
        for (int o = 0; o < HO; ++o) {
            float a[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) a[q] = 0.f;
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                const float wk = win.w[k];
#pragma unroll
                for (int q = 0; q < Q; ++q) a[q] += wk * p[q][o + k];
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) s_h[q][r][c0 + o] = a[q];
        }
    }
}

// columns: thread t's VO vertically adjacent outputs, rows (t / TW) VO + o of column t % TW of the tile (blur_out_row / _col), as
// v[o][0 .. Q).  Computed whether or not the output lies inside the image (LDS holds zeros there): the caller tests that.
template <int TW, int TH, int THREADS, int VO, int Q>
__device__ __forceinline__ void blur_cols(const RefineWindow& win, const float (&s_h)[Q][TH + 2 * RH][TW + 1], float (&v)[VO][Q])
{
    static_assert(TW * (TH / VO) == THREADS, "one work item per thread");
    const int tx = threadIdx.x % TW, ty0 = (threadIdx.x / TW) * VO;
    float col[Q][RW + VO - 1];
#pragma unroll
    for (int k = 0; k < RW + VO - 1; ++k)
#pragma unroll
        for (int q = 0; q < Q; ++q) col[q][k] = s_h[q][ty0 + k][tx];
#pragma unroll
    for (int o = 0; o < VO; ++o) {
#pragma unroll
        for (int q = 0; q < Q; ++q) v[o][q] = 0.f;
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            const float wk = win.w[k];
#pragma unroll
            for (int q = 0; q < Q; ++q) v[o][q] += wk * col[q][o + k];
        }
    }
}
template <int TW, int VO> __device__ __forceinline__ int blur_out_row(int o) { return (threadIdx.x / TW) * VO + o; }
template <int TW> __device__ __forceinline__ int blur_out_col() { return threadIdx.x % TW; }

// the SSIM map value m = A B / (C D).  RECIPROCAL: A B * (1 / (C D)), two roundings, as the refinement forward has always formed
// it; the evaluation divides once.  Both are pinned bit for bit by their callers' tests, so each keeps its form.
template <bool RECIPROCAL>
__device__ __forceinline__ float ssim_value(const SsimStats& st)
{
    const float A = 2.0f * st.mu1 * st.mu2 + SSIM_C1, B = 2.0f * st.sig12 + SSIM_C2;
    // mu1^2 + mu2^2 contracts to one fma either way round, and the two ways round differ by an ulp: the way is written down
    const float Cc = fmaf(st.mu1, st.mu1, st.mu2 * st.mu2) + SSIM_C1, D = st.sig1 + st.sig2 + SSIM_C2;
    if constexpr (RECIPROCAL) return A * B * (1.0f / (Cc * D));
    else return A * B / (Cc * D);
}

__global__ void __launch_bounds__(256)
refine_fwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, RefineWindow win,
                  float* __restrict__ dm_dmu1, float* __restrict__ dm_ds1, float* __restrict__ dm_ds12,
                  double* __restrict__ partial /*[blocks][2]: sum m, sum |x-y|*/)
{
    __shared__ float s_in[2][FH + 2 * RH][FW + 2 * RH + 1];   // x - shift, y - shift
    __shared__ float s_h[5][FH + 2 * RH][FW + 1];
    __shared__ double s_red[256 / WAVE][2];
    const int x0 = blockIdx.x * FW, y0 = blockIdx.y * FH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float shift = tile_shift(gt + plane, H, W, y0, x0, FH, FW);   // SHIFTED MOMENTS
    double sums[2] = {0.0, 0.0};   // m, |x - y|
    blur_load_tile<FW, FH, 256>(s_in, H, W, y0, x0, [&](size_t o, bool own, float (&v)[2]) {
        const float xr = img[plane + o], yr = gt[plane + o];
        v[0] = xr - shift;
        v[1] = yr - shift;
        if (own) sums[1] += (double)fabsf(xr - yr);
    });
    __syncthreads();
    blur_rows<FW, FH, 256, 4, true>(win, s_in, s_h);
    __syncthreads();
    const int gx = x0 + blur_out_col<FW>();
    double cover[2];   // ahead of the column pass: its eleven weights in double are dead before the pass needs its registers
#pragma unroll
    for (int o = 0; o < 2; ++o) cover[o] = ssim_cover(win, y0 + blur_out_row<FW, 2>(o), gx, H, W);
    float v[2][5];
    blur_cols<FW, FH, 256>(win, s_h, v);
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int gy = y0 + blur_out_row<FW, 2>(o);
        if (gy >= H || gx >= W) continue;
        const float C1 = SSIM_C1, C2 = SSIM_C2;
        const SsimStats st = ssim_stats(v[o], shift, cover[o]);
        const float mu1 = st.mu1, mu2 = st.mu2, sig1 = st.sig1, sig2 = st.sig2, sig12 = st.sig12;
        const size_t oo = plane + (size_t)gy * W + gx;
        // the partials in double, rounded once: the two halves of dm/dmu1 cancel where x is near y, and in float32 the
        // roundings of A, B, C and D alone put a one-pixel image's gradient an ulp off
        const double Ad = 2.0 * (double)mu1 * (double)mu2 + (double)C1, Bd = 2.0 * (double)sig12 + (double)C2;
        const double Cd = (double)mu1 * (double)mu1 + (double)mu2 * (double)mu2 + (double)C1;
        const double Dd = (double)sig1 + (double)sig2 + (double)C2;
        const double icdd = 1.0 / (Cd * Dd);
        dm_dmu1[oo] = (float)((2.0 * (double)mu2 * (Bd - Ad) * Cd * Dd - Ad * Bd * 2.0 * (double)mu1 * (Dd - Cd)) * icdd * icdd);
        dm_ds1[oo] = (float)(-Ad * Bd * icdd * icdd * Cd);
        dm_ds12[oo] = (float)(2.0 * Ad * icdd);
        sums[0] += (double)ssim_value<true>(st);
    }
    block_sum<256>(sums, s_red);
    if (threadIdx.x == 0) {
        const size_t bid = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * bid] = block_total(s_red, 0);
        partial[2 * bid + 1] = block_total(s_red, 1);
    }
}

// the loss values out of refine_fwd_kernel's per-block partial sums (a fixed order: deterministic): run by ONE block of
// refine_bwd_kernel — the values depend on the forward launch only, and a launch of their own cost the stream 4.7 us
__device__ __forceinline__ void refine_finish_block(int blocks, double n_total, float lambda, const double* __restrict__ partial,
                                                    float* __restrict__ out /*[3] = l1, ssim, loss*/)
{
    __shared__ double s_red[LOSS_BLOCK / WAVE][2];
    double t[2];   // sum m, sum |x - y|
    partials_block_sum<LOSS_BLOCK>(blocks, partial, s_red, t);
    if (threadIdx.x == 0) {
        const double ssim = t[0] / n_total, l1 = t[1] / n_total;
        out[0] = (float)l1;
        out[1] = (float)ssim;
        out[2] = (float)((1.0 - (double)lambda) * l1 + (double)lambda * (1.0 - ssim));
    }
}

__global__ void __launch_bounds__(256)
refine_bwd_kernel(int H, int W, float n_total, float lambda, const float* __restrict__ img,
                  const float* __restrict__ gt, RefineWindow win, const float* __restrict__ dm_dmu1,
                  const float* __restrict__ dm_ds1, const float* __restrict__ dm_ds12, float* __restrict__ g_img,
                  int blocks, double n_total_d, const double* __restrict__ partial, float* __restrict__ out)
{
    __shared__ float s_in[3][FH + 2 * RH][FW + 2 * RH + 1];   // dm/dmu1, dm/ds1, dm/ds12
    __shared__ float s_h[3][FH + 2 * RH][FW + 1];
    const int x0 = blockIdx.x * FW, y0 = blockIdx.y * FH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    blur_load_tile<FW, FH, 256>(s_in, H, W, y0, x0, [&](size_t o, bool, float (&v)[3]) {
        v[0] = dm_dmu1[plane + o];
        v[1] = dm_ds1[plane + o];
        v[2] = dm_ds12[plane + o];
    });
    __syncthreads();
    blur_rows<FW, FH, 256, 4, false>(win, s_in, s_h);
    __syncthreads();
    float b[2][3];
    blur_cols<FW, FH, 256>(win, s_h, b);
    const int gx = x0 + blur_out_col<FW>();
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int gy = y0 + blur_out_row<FW, 2>(o);
        if (gy >= H || gx >= W) continue;
        const size_t oo = plane + (size_t)gy * W + gx;
        const float x = img[oo], y = gt[oo];
        const float inv_n = 1.0f / n_total;
        g_img[oo] = (1.0f - lambda) * sgn(x - y) * inv_n - lambda * inv_n * (b[o][0] + 2.0f * x * b[o][1] + y * b[o][2]);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) refine_finish_block(blocks, n_total_d, lambda, partial, out);
}

static RefineWindow refine_window()
{
    // loss_utils.py:42-49: exp in double -> float32 tensor -> divided by its float32 sum
    RefineWindow win;
    float sum = 0.f;
    for (int k = 0; k < RW; ++k) {
        win.w[k] = (float)exp(-(double)((k - RH) * (k - RH)) / (2.0 * 1.5 * 1.5));
        sum += win.w[k];
    }
    for (int k = 0; k < RW; ++k) win.w[k] /= sum;
    double mass = 0.0;
    for (int k = 0; k < RW; ++k) mass += (double)win.w[k];
    win.mass = mass;
    return win;
}

// [three maps of C H W floats | block partials]
struct RefineWs { float* maps; double* partial; size_t bytes; };
static RefineWs refine_layout(void* workspace, int32_t C, int32_t H, int32_t W)
{
    const size_t blocks = (size_t)((W + FW - 1) / FW) * ((H + FH - 1) / FH) * (size_t)C;
    RefineWs w;
    Carver c{workspace};
    w.maps = c.take<float>(3 * (size_t)C * H * W);
    w.partial = c.take<double>(blocks * 2);
    w.bytes = c.o;
    return w;
}

// ---------------------------------------------------------------------------------------------
// eval_rendering's per-frame metrics (utils/eval_utils.py:22-72):
//     image = clamp(render, 0, 1);  mask = gt > 0 (per element)
//     psnr  = 20 log10(1 / sqrt(mean_{mask} (image - gt)^2))          gaussian_splatting/utils/image_utils.py:19-21
//     ssim  = ssim(image, gt)                                          loss_utils.py:61-102 (same window as above)
// one pass over the frame: the tile loader clamps, the SSIM map is summed (its partial derivatives are not needed),
// and the masked squared error and the mask count ride in the same block partials (double, deterministic).
// ---------------------------------------------------------------------------------------------
constexpr int EVAL_SUMS = 3;   // sum ssim map, sum mask (x - y)^2, sum mask

__global__ void __launch_bounds__(RT * RT)
eval_metrics_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, RefineWindow win,
                    double* __restrict__ partial /*[blocks][EVAL_SUMS]*/)
{
    __shared__ float s_in[2][RT + 2 * RH][RT + 2 * RH + 1];   // clamped x - shift, y - shift
    __shared__ float s_h[5][RT + 2 * RH][RT + 1];
    __shared__ double s_red[RT * RT / WAVE][EVAL_SUMS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RT, y0 = blockIdx.y * RT;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float shift = tile_shift(gt + plane, H, W, y0, x0, RT, RT);   // SHIFTED MOMENTS
    double acc[EVAL_SUMS] = {0.0, 0.0, 0.0};
    blur_load_tile<RT, RT, RT * RT>(s_in, H, W, y0, x0, [&](size_t o, bool own, float (&v)[2]) {
        const float xr = fminf(fmaxf(img[plane + o], 0.0f), 1.0f);   // torch.clamp(rendering, 0.0, 1.0)
        const float yr = gt[plane + o];
        v[0] = xr - shift;
        v[1] = yr - shift;
        if (own && yr > 0.0f) {   // masked per element
            const float d = xr - yr;
            acc[1] += (double)(d * d);
            acc[2] += 1.0;
        }
    });
    __syncthreads();
    blur_rows<RT, RT, RT * RT, 1, true>(win, s_in, s_h);
    __syncthreads();
    const int gy = y0 + blur_out_row<RT, 1>(0), gx = x0 + blur_out_col<RT>();
    const double cover = ssim_cover(win, gy, gx, H, W);   // ahead of the column pass, as in refine_fwd_kernel
    float v[1][5];
    blur_cols<RT, RT, RT * RT>(win, s_h, v);
    if (gy < H && gx < W) acc[0] = (double)ssim_value<false>(ssim_stats(v[0], shift, cover));
    block_sum<RT * RT>(acc, s_red);
    if (tid < EVAL_SUMS) {
        const size_t bid = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[EVAL_SUMS * bid + tid] = block_total(s_red, tid);
    }
}

__global__ void __launch_bounds__(LOSS_BLOCK)
eval_metrics_finish_kernel(int blocks, double n_total, const double* __restrict__ partial,
                           float* __restrict__ out /*[4] = psnr, ssim, masked mse, mask count*/)
{
    __shared__ double s_red[LOSS_BLOCK / WAVE][EVAL_SUMS];
    double t[EVAL_SUMS];
    partials_block_sum<LOSS_BLOCK>(blocks, partial, s_red, t);
    if (threadIdx.x == 0) {
        const double mse = t[2] > 0 ? t[1] / t[2] : 0.0 / 0.0;     // an empty mask: the reference's mean over nothing is NaN
        out[0] = (float)(20.0 * log10(1.0 / sqrt(mse)));
        out[1] = (float)(t[0] / n_total);
        out[2] = (float)mse;
        out[3] = (float)t[2];
    }
}

static size_t eval_metrics_workspace_bytes(int32_t C, int32_t H, int32_t W)
{
    const size_t blocks = (size_t)((W + RT - 1) / RT) * ((H + RT - 1) / RT) * (size_t)C;
    return blocks * EVAL_SUMS * sizeof(double);
}

static int launch_eval_metrics(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, float* out, void* workspace,
                        hipStream_t stream)
{
    const dim3 grid((W + RT - 1) / RT, (H + RT - 1) / RT, C);
    const int blocks = (int)(grid.x * grid.y * grid.z);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(eval_metrics_kernel, grid, dim3(RT * RT), 0, stream, H, W, image, gt, refine_window(), partial);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_metrics_finish_kernel, dim3(1), dim3(LOSS_BLOCK), 0, stream, blocks, (double)C * H * W, partial, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

static int launch_refinement_loss(int32_t C, int32_t H, int32_t W, float lambda, const float* image, const float* gt,
                           float* g_image, float* out, void* workspace, hipStream_t stream)
{
    const size_t n = (size_t)C * H * W;
    const RefineWs w = refine_layout(workspace, C, H, W);
    float* maps = w.maps;
    double* partial = w.partial;
    const dim3 grid((W + FW - 1) / FW, (H + FH - 1) / FH, C);
    const int blocks = (int)(grid.x * grid.y * grid.z);
    const RefineWindow win = refine_window();
    hipLaunchKernelGGL(refine_fwd_kernel, grid, dim3(256), 0, stream, H, W, image, gt, win, maps, maps + n,
                       maps + 2 * n, partial);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(refine_bwd_kernel, grid, dim3(256), 0, stream, H, W, (float)n, lambda, image, gt, win, maps,
                       maps + n, maps + 2 * n, g_image, blocks, (double)n, partial, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr

using namespace sr;

extern "C" {

size_t splatraster_mapping_loss_workspace_bytes(int32_t pixels) { return pixels > 0 ? mapping_loss_workspace_bytes(pixels) : 0; }

int splatraster_mapping_loss(int32_t pixels, const float* image, const float* depth, const float* marker,
                             const float* gt_image, const float* gt_depth, const float* kp,
                             float rgb_boundary_threshold, const float* exposure, float* g_image, float* g_depth,
                             float* g_marker, float* out, void* workspace, void* stream)
{
    if (pixels <= 0) return SPLATRASTER_ERR_BAD_ARG;
    if (!image || !depth || !marker || !gt_image || !gt_depth || !kp || !g_image || !g_depth || !g_marker || !out ||
        !workspace)
        return SPLATRASTER_ERR_BAD_ARG;
    return launch_mapping_loss(pixels, image, depth, marker, gt_image, gt_depth, kp, rgb_boundary_threshold, exposure,
                               g_image, g_depth, g_marker, out, workspace, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_mapping_loss_window(int32_t n_views, int32_t pixels, const splatraster_loss_view* views,
                                    float rgb_boundary_threshold, float* out, void* workspace, void* stream)
{
    if (pixels <= 0 || n_views < 1 || n_views > SPLATRASTER_MAX_WINDOW_VIEWS || !views || !out || !workspace)
        return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < n_views; ++v) {
        const splatraster_loss_view& w = views[v];
        if (!w.image || !w.depth || !w.marker || !w.gt_image || !w.gt_depth || !w.kp || !w.g_image || !w.g_depth || !w.g_marker)
            return SPLATRASTER_ERR_BAD_ARG;
    }
    return launch_mapping_loss_window(n_views, pixels, views, rgb_boundary_threshold, out, workspace,
                                      reinterpret_cast<hipStream_t>(stream));
}

size_t splatraster_refinement_loss_workspace_bytes(int32_t channels, int32_t height, int32_t width)
{
    if (channels <= 0 || height <= 0 || width <= 0) return 0;
    return refine_layout(nullptr, channels, height, width).bytes;
}

int splatraster_refinement_loss(int32_t channels, int32_t height, int32_t width, float lambda_dssim,
                                const float* image, const float* gt, float* g_image, float* out, void* workspace,
                                void* stream)
{
    if (channels <= 0 || height <= 0 || width <= 0) return SPLATRASTER_ERR_BAD_ARG;
    if (!image || !gt || !g_image || !out || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    return launch_refinement_loss(channels, height, width, lambda_dssim, image, gt, g_image, out, workspace,
                                  reinterpret_cast<hipStream_t>(stream));
}

size_t splatraster_eval_metrics_workspace_bytes(int32_t channels, int32_t height, int32_t width)
{
    if (channels <= 0 || height <= 0 || width <= 0) return 0;
    return eval_metrics_workspace_bytes(channels, height, width);
}

int splatraster_eval_metrics(int32_t channels, int32_t height, int32_t width, const float* render, const float* gt, float* out,
                             void* workspace, void* stream)
{
    if (channels <= 0 || height <= 0 || width <= 0) return SPLATRASTER_ERR_BAD_ARG;
    if (!render || !gt || !out || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    return launch_eval_metrics(channels, height, width, render, gt, out, workspace, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
