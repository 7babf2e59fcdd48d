// image_ops.hip — frame preparation: the Scharr image gradients, the validity mask, Camera.compute_grad_mask for both dataset
// types and the masked medians of get_median_depth (utils/utils.py:4-38, 85-96; utils/camera_utils.py:145-172), several frames
// per launch, nothing read back.  Definition: include/splatraster.h (splatraster_image_gradient, splatraster_grad_mask,
// splatraster_masked_median) and INTEGRATION.md §23.
//
// gfx950 shape.  Three kernels.
//  * img_gradient_kernel: one lane per pixel of a rectangle of a plane (64 x 4 lanes: a wave reads rows), grid z = plane.  It writes
//    the two gradients and the validity mask (the drop-in image_gradient / image_gradient_mask), or the intensity
//    sqrt((gv valid)^2 + (gh valid)^2) of the gray image (the frame-median branch, the first pass of oversized Replica blocks, and
//    the remainder rows / columns of the Replica branch, which keep the raw intensity).
//  * img_block_mask_kernel: the Replica branch, one workgroup per (block, frame) on a 32 x 32 x N grid.  The fused instantiations
//    stage the reflect-padded (bh + 2) x (bw + 2) gray halo in LDS, compute the block's n = bh bw intensities into LDS and select
//    the lower median there: the values are >= +0 or NaN, so their bit patterns are already ordered; four 8-bit digit passes, each
//    an LDS histogram of the values that still match the prefix, then one wave scans the 256 counts and picks the digit.  Only one
//    order statistic is needed, so nothing is sorted.  Two sizes: n <= 2048 in 19 KB (256 lanes; a 1080p block has 1 980 pixels,
//    several workgroups share a CU) and n <= 16 384 in 145 KB of the CU's 160 KB (1024 lanes; a 4096 x 4096 frame).  Beyond that
//    (or a halo beyond 20 480 words: blocks thinner than 1 : 60) the instantiation without LDS arrays reads the block's intensities,
//    written by img_gradient_kernel, from global memory in every pass.  splatraster_debug_image_ops_path names the path of a shape.
//  * img_select_hist_kernel / img_select_pick_kernel: the k-th order statistic of up to 2^31 values per frame under the
//    get_median_depth predicate.  Order-preserving keys from the float bits (negative values: all bits flipped; others: the sign
//    bit set), four 8-bit digit passes, each a per-workgroup LDS histogram flushed with 256 global atomics; after each pass one wave
//    per frame picks the digit and the remaining rank, so the count of selected elements, k = (count - 1) / 2 and the result never
//    leave the device.  The first pass also leaves per-workgroup double sums of v and v^2; the last pick adds them in workgroup
//    order (deterministic) for the unbiased standard deviation.
// Compiled without FP contraction: the nine taps are summed row-major, every product and sum rounding on its own, which
// tests/image_ops_reference.py restates bit for bit.
#include "common.h"
#include "scan.h"

#include <math.h>

namespace sr {

constexpr int IMG_THREADS = 256;
constexpr int IMG_ROWS = 4;              // a gradient workgroup: 64 x 4 pixels
constexpr int IMG_BLOCKS = 32;           // the Replica branch's blocks per side
constexpr int IMG_SMALL_N = 2048, IMG_SMALL_HALO = 2560;
constexpr int IMG_BIG_N = 16384, IMG_BIG_HALO = 20480, IMG_BIG_THREADS = 1024;
constexpr int IMG_MAX_SIDE = 65536;      // H, W: a block's pixel count stays an int
constexpr int IMG_MAX_PLANES = 65535;    // gridDim.z
constexpr int64_t SEL_MAX_N = (int64_t)1 << 31;
constexpr int SEL_ITEMS = 16, SEL_MAX_BLOCKS = 512;
constexpr int SEL_STATE_WORDS = 4;       // prefix (key space), remaining rank, count, NaNs among the selected
enum { IMG_PATH_NONE = 0, IMG_PATH_LDS_SMALL = 1, IMG_PATH_LDS_BIG = 2, IMG_PATH_GLOBAL = 3 };

static int image_ops_path(int32_t H, int32_t W)
{
    if (H < IMG_BLOCKS || W < IMG_BLOCKS || H > IMG_MAX_SIDE || W > IMG_MAX_SIDE) return IMG_PATH_NONE;
    const int64_t bh = H / IMG_BLOCKS, bw = W / IMG_BLOCKS;
    const int64_t n = bh * bw, halo = (bh + 2) * (bw + 2);
    if (n <= IMG_SMALL_N && halo <= IMG_SMALL_HALO) return IMG_PATH_LDS_SMALL;
    if (n <= IMG_BIG_N && halo <= IMG_BIG_HALO) return IMG_PATH_LDS_BIG;
    return IMG_PATH_GLOBAL;
}

// reflect padding by one pixel: the border itself is not repeated
__device__ __forceinline__ int img_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// pixel `at` of a plane: the gray value ((r + g) + b) / 3 of a three-plane image, or the plane itself
__device__ __forceinline__ float img_pixel(const float* __restrict__ img, bool gray, int64_t plane, int64_t at)
{
    if (!gray) return img[at];
    return ((img[at] + img[at + plane]) + img[at + 2 * plane]) / 3.0f;   // correctly rounded: no fast-math
}

// the 3 x 3 neighbourhood p (row-major) -> grad_v, grad_h (cross-correlation, scaled by 1/32) and validity.  The zero taps are
// multiplied and added like the others: 0 * NaN is NaN, as in conv2d
__device__ __forceinline__ void img_scharr(const float* p, float eps, float* gv, float* gh, bool* valid)
{
    constexpr float wv[9] = {3.f, 10.f, 3.f, 0.f, 0.f, 0.f, -3.f, -10.f, -3.f};
    constexpr float wh[9] = {3.f, 0.f, -3.f, 10.f, 0.f, -10.f, 3.f, 0.f, -3.f};
    float av = wv[0] * p[0], ah = wh[0] * p[0];
    bool ok = fabsf(p[0]) > eps;
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        av = av + wv[k] * p[k];
        ah = ah + wh[k] * p[k];
        ok = ok && fabsf(p[k]) > eps;
    }
    *gv = 0.03125f * av;
    *gh = 0.03125f * ah;
    *valid = ok;
}

__device__ __forceinline__ float img_intensity(float gv, float gh, bool valid)
{
    const float m = valid ? 1.f : 0.f;
    const float a = gv * m, b = gh * m;
    return sqrtf(a * a + b * b);   // correctly rounded (hipcc's default for fp32 sqrt and divide), unlike __fsqrt_rn's native form
}

// one lane per pixel of the rectangle [x0, x0 + rw) x [y0, y0 + rh) of every plane (grid z)
__global__ void __launch_bounds__(IMG_THREADS)
img_gradient_kernel(int H, int W, int x0, int y0, int rw, int rh, const float* __restrict__ img, int gray, float eps,
                    float* __restrict__ grad_v, float* __restrict__ grad_h, uint8_t* __restrict__ valid_out,
                    float* __restrict__ intensity, float* __restrict__ intensity2)
{
    const int rx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ry = blockIdx.y * IMG_ROWS + (threadIdx.x >> 6);
    if (rx >= rw || ry >= rh) return;
    const int x = x0 + rx, y = y0 + ry;
    const int64_t plane = (int64_t)H * W;
    const float* src = img + (int64_t)blockIdx.z * plane * (gray ? 3 : 1);
    float p[9];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int64_t row = (int64_t)img_reflect(y + dy - 1, H) * W;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) p[dy * 3 + dx] = img_pixel(src, gray != 0, plane, row + img_reflect(x + dx - 1, W));
    }
    float gv, gh;
    bool ok;
    img_scharr(p, eps, &gv, &gh, &ok);
    const int64_t at = (int64_t)blockIdx.z * plane + (int64_t)y * W + x;
    if (grad_v) grad_v[at] = gv;
    if (grad_h) grad_h[at] = gh;
    if (valid_out) valid_out[at] = ok ? 1 : 0;
    if (intensity || intensity2) {
        const float v = img_intensity(gv, gh, ok);
        if (intensity) intensity[at] = v;
        if (intensity2) intensity2[at] = v;
    }
}

// The Replica branch: workgroup (c, r, f) owns block (r, c) of frame f.  NCAP > 0: the fused form (halo and intensities in LDS);
// NCAP == 0: the block's intensities are read from xg, where img_gradient_kernel wrote them.
template <int THREADS, int NCAP, int HCAP>
__global__ void __launch_bounds__(THREADS)
img_block_mask_kernel(int H, int W, int bh, int bw, const float* __restrict__ img, float eps, float edge_threshold,
                      const float* __restrict__ xg, float* __restrict__ out, float* __restrict__ intensity,
                      float* __restrict__ thresholds)
{
    constexpr bool FUSED = NCAP > 0;
    __shared__ float s_halo[FUSED ? HCAP : 1];
    __shared__ float s_x[FUSED ? NCAP : 1];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[2];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * bw, y0 = blockIdx.y * bh, n = bh * bw;
    const int64_t plane = (int64_t)H * W;
    const int64_t frame = (int64_t)blockIdx.z * plane;

    if constexpr (FUSED) {
        const int hw = bw + 2, hn = (bh + 2) * hw;
        const float* src = img + 3 * frame;
        for (int i = tid; i < hn; i += THREADS) {
            const int hy = i / hw, hx = i - hy * hw;
            s_halo[i] = img_pixel(src, true, plane, (int64_t)img_reflect(y0 + hy - 1, H) * W + img_reflect(x0 + hx - 1, W));
        }
        __syncthreads();
        for (int i = tid; i < n; i += THREADS) {
            const int by = i / bw, bx = i - by * bw;
            float p[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) p[dy * 3 + dx] = s_halo[(by + dy) * hw + bx + dx];
            float gv, gh;
            bool ok;
            img_scharr(p, eps, &gv, &gh, &ok);
            const float v = img_intensity(gv, gh, ok);
            s_x[i] = v;
            if (intensity) intensity[frame + (int64_t)(y0 + by) * W + x0 + bx] = v;
        }
    }
    auto value = [&](int i) -> float {
        if constexpr (FUSED) return s_x[i];
        const int by = i / bw;
        return xg[frame + (int64_t)(y0 + by) * W + x0 + (i - by * bw)];
    };

    // lower median: element (n - 1) / 2 of the ascending order, by radix select over the bits (every value is >= +0 or NaN; s_x is
    // complete behind the select's first barrier).  The NaN vote is the barrier behind the select's first pass.
    int nan = 0, any_nan = 0;
    const uint32_t prefix = radix_select_block<THREADS, false>(
        (uint32_t)n,
        [&](uint32_t i) {
            const float v = value((int)i);
            nan |= v != v;
            return __float_as_uint(v);
        },
        (uint32_t)(n - 1) / 2, s_hist, s_sel, nullptr, [&]() { any_nan = __syncthreads_or(nan); });
    // block[block > t] = 1; block[block <= t] = 0: a 1 written by the first statement is zeroed by the second when t >= 1; both
    // comparisons are false everywhere when t is NaN (a NaN in the block, or inf * 0)
    const float t = any_nan ? __uint_as_float(0x7FC00000u) : __uint_as_float(prefix) * edge_threshold;
    if (tid == 0 && thresholds) thresholds[((int64_t)blockIdx.z * IMG_BLOCKS + blockIdx.y) * IMG_BLOCKS + blockIdx.x] = t;
    const bool keep = t != t, below_one = t < 1.0f;
    for (int i = tid; i < n; i += THREADS) {
        const int by = i / bw, bx = i - by * bw;
        const float v = value(i);
        out[frame + (int64_t)(y0 + by) * W + x0 + bx] = keep ? v : ((v > t && below_one) ? 1.0f : 0.0f);
    }
}

// out = x > median * edge_threshold over whole frames (the other dataset types)
__global__ void __launch_bounds__(IMG_THREADS)
img_threshold_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ median, float edge_threshold,
                     float* __restrict__ out_f, uint8_t* __restrict__ out_u8, float* __restrict__ thresholds)
{
    const int f = blockIdx.y;
    const float t = median[f] * edge_threshold;
    if (blockIdx.x == 0 && threadIdx.x == 0 && thresholds) thresholds[f] = t;
    for (int64_t i = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IMG_THREADS) {
        const bool on = x[(int64_t)f * n + i] > t;
        if (out_f) out_f[(int64_t)f * n + i] = on ? 1.0f : 0.0f;
        if (out_u8) out_u8[(int64_t)f * n + i] = on ? 1 : 0;
    }
}

// ---- masked frame select ---------------------------------------------------------------------------------------------------------

struct SelWs {
    uint32_t* hist;     // [N][4][256]
    uint32_t* state;    // [N][SEL_STATE_WORDS]
    double* partials;   // [N][blocks][2]
    size_t zero_bytes;  // hist + state: cleared before the first pass
    size_t total;
};

static int sel_blocks(int64_t n)
{
    const int64_t b = (n + (int64_t)IMG_THREADS * SEL_ITEMS - 1) / ((int64_t)IMG_THREADS * SEL_ITEMS);
    return (int)(b < 1 ? 1 : (b > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : b));
}

static SelWs sel_layout(void* workspace, int32_t N, int64_t n)
{
    SelWs w;
    Carver c{workspace};
    w.hist = c.take<uint32_t>((size_t)N * 4 * 256);
    w.state = c.take<uint32_t>((size_t)N * SEL_STATE_WORDS);
    w.zero_bytes = c.o;
    w.partials = c.take<double>((size_t)N * sel_blocks(n) * 2);
    w.total = c.o;
    return w;
}

__device__ __forceinline__ double sel_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

__global__ void __launch_bounds__(IMG_THREADS)
img_select_hist_kernel(int64_t n, const float* __restrict__ values, int positive_only, const float* __restrict__ opacity,
                       float opacity_min, const uint8_t* __restrict__ mask, int pass, uint32_t* __restrict__ state_all,
                       uint32_t* __restrict__ hist_all, double* __restrict__ partials, uint8_t* __restrict__ valid_out)
{
    __shared__ uint32_t s_hist[256];
    __shared__ double s_sum[2 * (IMG_THREADS / 64)];
    const int tid = threadIdx.x, f = blockIdx.y;
    uint32_t* state = state_all + (int64_t)f * SEL_STATE_WORDS;
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = pass ? state[0] : 0u;
    const uint32_t hi = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
    s_hist[tid] = 0;
    __syncthreads();
    double sum = 0.0, sq = 0.0;
    uint32_t nans = 0;
    const int64_t base = (int64_t)f * n;
    for (int64_t i = (int64_t)blockIdx.x * IMG_THREADS + tid; i < n; i += (int64_t)gridDim.x * IMG_THREADS) {
        const float v = values[base + i];
        bool sel = !positive_only || v > 0.0f;
        if (opacity) sel = sel && opacity[base + i] > opacity_min;
        if (mask) sel = sel && mask[base + i] != 0;
        if (pass == 0 && valid_out) valid_out[base + i] = sel ? 1 : 0;
        if (!sel) continue;
        if (pass == 0) {
            nans += v != v;
            sum += (double)v;
            sq += (double)v * (double)v;
        }
        const uint32_t key = float_order_key(v);
        if ((key & hi) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (s_hist[tid]) atomicAdd(&hist_all[((int64_t)f * 4 + pass) * 256 + tid], s_hist[tid]);
    if (pass == 0) {
        if (nans) atomicAdd(&state[3], nans);
        sum = sel_wave_sum(sum);
        sq = sel_wave_sum(sq);
        if ((tid & 63) == 0) {
            s_sum[2 * (tid >> 6)] = sum;
            s_sum[2 * (tid >> 6) + 1] = sq;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0, b = 0.0;
            for (int w = 0; w < IMG_THREADS / 64; ++w) {
                a += s_sum[2 * w];
                b += s_sum[2 * w + 1];
            }
            double* dst = partials + ((int64_t)f * gridDim.x + blockIdx.x) * 2;
            dst[0] = a;
            dst[1] = b;
        }
    }
}

// one wave per frame: the digit of this pass and the rank left; the last pass writes the results
__global__ void __launch_bounds__(64)
img_select_pick_kernel(int pass, int blocks, uint32_t* __restrict__ state_all, const uint32_t* __restrict__ hist_all,
                       const double* __restrict__ partials, float* __restrict__ median, float* __restrict__ std_out,
                       int64_t* __restrict__ count)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    uint32_t* state = state_all + (int64_t)f * SEL_STATE_WORDS;
    const int shift = 24 - 8 * pass;
    uint32_t digit, rank, total;
    const uint32_t prefix_in = pass ? state[0] : 0u, k_in = pass ? state[1] : 0u;
    radix_pick<false>(hist_all + ((int64_t)f * 4 + pass) * 256, pass == 0, k_in, &digit, &rank, &total);
    const uint32_t prefix = prefix_in | (digit << shift);
    const uint32_t cnt = pass == 0 ? total : state[2];
    __syncthreads();   // every lane has read the state
    if (lane == 0) {
        state[0] = prefix;
        state[1] = rank;
        if (pass == 0) state[2] = total;
    }
    if (pass != 3) return;
    const float nanf_ = __uint_as_float(0x7FC00000u);
    const bool none = cnt == 0 || state[3] != 0;
    if (lane == 0) {
        median[f] = none ? nanf_ : float_from_order_key(prefix);
        if (count) count[f] = (int64_t)cnt;
    }
    if (std_out) {
        double a = 0.0, b = 0.0;
        for (int w = lane; w < blocks; w += 64) {
            a += partials[((int64_t)f * blocks + w) * 2];
            b += partials[((int64_t)f * blocks + w) * 2 + 1];
        }
        a = sel_wave_sum(a);
        b = sel_wave_sum(b);
        if (lane == 0) {
            // unbiased: (sum v^2 - (sum v)^2 / n) / (n - 1); one element: 0 / 0 = NaN, as torch.std
            const double nn = (double)cnt;
            double var = (b - a * a / nn) / (nn - 1.0);
            if (var < 0.0) var = 0.0;
            std_out[f] = cnt == 0 ? nanf_ : (float)sqrt(var);
        }
    }
}

static int launch_frame_select(int32_t N, int64_t n, const float* values, int positive_only, const float* opacity, float opacity_min,
                               const uint8_t* mask, float* median, float* std_out, int64_t* count, uint8_t* valid, void* workspace,
                               hipStream_t stream)
{
    const SelWs w = sel_layout(workspace, N, n);
    const int blocks = sel_blocks(n);
    SR_HIP_CHECK(hipMemsetAsync(workspace, 0, w.zero_bytes, stream));
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(img_select_hist_kernel, dim3(blocks, N), dim3(IMG_THREADS), 0, stream, n, values, positive_only, opacity,
                           opacity_min, mask, pass, w.state, w.hist, w.partials, valid);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(img_select_pick_kernel, dim3(N), dim3(64), 0, stream, pass, blocks, w.state, (const uint32_t*)w.hist,
                           (const double*)w.partials, median, std_out, count);
        SR_LAUNCH_CHECK();
    }
    return SPLATRASTER_OK;
}

static int launch_gradient(int32_t planes, int H, int W, int x0, int y0, int rw, int rh, const float* img, int gray, float eps,
                           float* grad_v, float* grad_h, uint8_t* valid, float* intensity, float* intensity2, hipStream_t stream)
{
    if (rw <= 0 || rh <= 0) return SPLATRASTER_OK;
    hipLaunchKernelGGL(img_gradient_kernel, dim3((rw + 63) / 64, (rh + IMG_ROWS - 1) / IMG_ROWS, planes), dim3(IMG_THREADS), 0, stream,
                       H, W, x0, y0, rw, rh, img, gray, eps, grad_v, grad_h, valid, intensity, intensity2);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

static bool bad_frame(int32_t N, int32_t H, int32_t W)
{
    return N < 1 || N > IMG_MAX_PLANES || H < 2 || W < 2 || H > IMG_MAX_SIDE || W > IMG_MAX_SIDE;
}

// what splatraster_grad_mask needs behind the caller's buffers: [frame select | medians N | intensities N H W]
struct MaskWs {
    void* select;                // sel_layout's buffer (GLOBAL mode), else null
    float *medians, *intensity;  // null where the mode / the caller's own intensity plane leaves the section out
    size_t total;
};

static MaskWs mask_layout(void* workspace, int32_t N, int32_t H, int32_t W, int mode, bool have_intensity)
{
    MaskWs m{};
    Carver c{workspace};
    const int64_t n = (int64_t)H * W;
    const bool scratch = !have_intensity && (mode == SPLATRASTER_GRAD_MASK_GLOBAL || image_ops_path(H, W) == IMG_PATH_GLOBAL);
    if (mode == SPLATRASTER_GRAD_MASK_GLOBAL) {
        m.select = c.take<char>(sel_layout(nullptr, N, n).total);
        m.medians = c.take<float>((size_t)N);
    }
    if (scratch) m.intensity = c.take<float>((size_t)N * n);
    m.total = c.o;
    return m;
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_debug_image_ops_path(int32_t H, int32_t W) { return image_ops_path(H, W); }

int splatraster_image_gradient(int32_t N, int32_t C, int32_t H, int32_t W, const float* image, float eps, float* grad_v, float* grad_h,
                               uint8_t* valid, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (C < 1 || bad_frame(N, H, W) || (int64_t)N * C > IMG_MAX_PLANES || !image) return SPLATRASTER_ERR_BAD_ARG;
    if (!grad_v && !grad_h && !valid) return SPLATRASTER_ERR_BAD_ARG;
    if (!(eps >= 0.0f)) return SPLATRASTER_ERR_BAD_ARG;
    return launch_gradient(N * C, H, W, 0, 0, W, H, image, 0, eps, grad_v, grad_h, valid, nullptr, nullptr, stream);
}

int splatraster_grad_mask_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t mode, int32_t have_intensity, size_t* bytes)
{
    if (bytes) *bytes = 0;
    if (!bytes || bad_frame(N, H, W)) return SPLATRASTER_ERR_BAD_ARG;
    if (mode != SPLATRASTER_GRAD_MASK_REPLICA && mode != SPLATRASTER_GRAD_MASK_GLOBAL) return SPLATRASTER_ERR_BAD_ARG;
    if (mode == SPLATRASTER_GRAD_MASK_REPLICA && image_ops_path(H, W) == IMG_PATH_NONE) return SPLATRASTER_ERR_BAD_ARG;
    *bytes = mask_layout(nullptr, N, H, W, mode, have_intensity != 0).total;
    return SPLATRASTER_OK;
}

int splatraster_grad_mask(int32_t N, int32_t H, int32_t W, const float* images, float edge_threshold, float eps, int32_t mode,
                          int32_t out_u8, void* out, float* intensity, float* thresholds, void* workspace, size_t workspace_bytes,
                          void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (bad_frame(N, H, W) || !images || !out) return SPLATRASTER_ERR_BAD_ARG;
    if (mode != SPLATRASTER_GRAD_MASK_REPLICA && mode != SPLATRASTER_GRAD_MASK_GLOBAL) return SPLATRASTER_ERR_BAD_ARG;
    if (!(eps >= 0.0f) || edge_threshold != edge_threshold) return SPLATRASTER_ERR_BAD_ARG;
    const int path = image_ops_path(H, W);
    if (mode == SPLATRASTER_GRAD_MASK_REPLICA && path == IMG_PATH_NONE) return SPLATRASTER_ERR_BAD_ARG;   // an empty block: the reference raises
    if (mode == SPLATRASTER_GRAD_MASK_REPLICA && out_u8) return SPLATRASTER_ERR_UNSUPPORTED;   // the remainder keeps raw intensities
    const MaskWs m = mask_layout(workspace, N, H, W, mode, intensity != nullptr);
    if (m.total > 0 && (!workspace || workspace_bytes < m.total)) return SPLATRASTER_ERR_BAD_ARG;
    float* xs = intensity ? intensity : m.intensity;
    int st;

    if (mode == SPLATRASTER_GRAD_MASK_GLOBAL) {
        const int64_t n = (int64_t)H * W;
        float* medians = m.medians;
        if ((st = launch_gradient(N, H, W, 0, 0, W, H, images, 1, eps, nullptr, nullptr, nullptr, xs, nullptr, stream))) return st;
        if ((st = launch_frame_select(N, n, xs, 0, nullptr, 0.f, nullptr, medians, nullptr, nullptr, nullptr, m.select, stream))) return st;
        hipLaunchKernelGGL(img_threshold_kernel, dim3(sel_blocks(n), N), dim3(IMG_THREADS), 0, stream, n, (const float*)xs,
                           (const float*)medians, edge_threshold, out_u8 ? nullptr : reinterpret_cast<float*>(out),
                           out_u8 ? reinterpret_cast<uint8_t*>(out) : nullptr, thresholds);
        SR_LAUNCH_CHECK();
        return SPLATRASTER_OK;
    }

    const int bh = H / IMG_BLOCKS, bw = W / IMG_BLOCKS;
    float* outf = reinterpret_cast<float*>(out);
    const dim3 grid(IMG_BLOCKS, IMG_BLOCKS, N);
    if (path == IMG_PATH_LDS_SMALL) {
        hipLaunchKernelGGL((img_block_mask_kernel<IMG_THREADS, IMG_SMALL_N, IMG_SMALL_HALO>), grid, dim3(IMG_THREADS), 0, stream, H, W, bh,
                           bw, images, eps, edge_threshold, (const float*)nullptr, outf, intensity, thresholds);
    } else if (path == IMG_PATH_LDS_BIG) {
        hipLaunchKernelGGL((img_block_mask_kernel<IMG_BIG_THREADS, IMG_BIG_N, IMG_BIG_HALO>), grid, dim3(IMG_BIG_THREADS), 0, stream, H, W,
                           bh, bw, images, eps, edge_threshold, (const float*)nullptr, outf, intensity, thresholds);
    } else {
        if ((st = launch_gradient(N, H, W, 0, 0, W, H, images, 1, eps, nullptr, nullptr, nullptr, xs, nullptr, stream))) return st;
        hipLaunchKernelGGL((img_block_mask_kernel<IMG_BIG_THREADS, 0, 0>), grid, dim3(IMG_BIG_THREADS), 0, stream, H, W, bh, bw, images, eps,
                           edge_threshold, (const float*)xs, outf, (float*)nullptr, thresholds);
    }
    SR_LAUNCH_CHECK();
    // rows at or beyond 32 bh and columns at or beyond 32 bw keep the raw intensity
    float* also = path == IMG_PATH_GLOBAL ? nullptr : intensity;
    const int hb = IMG_BLOCKS * bh, wb = IMG_BLOCKS * bw;
    if ((st = launch_gradient(N, H, W, 0, hb, W, H - hb, images, 1, eps, nullptr, nullptr, nullptr, outf, also, stream))) return st;
    return launch_gradient(N, H, W, wb, 0, W - wb, hb, images, 1, eps, nullptr, nullptr, nullptr, outf, also, stream);
}

int splatraster_masked_median_workspace_bytes(int32_t N, int64_t n, size_t* bytes)
{
    if (bytes) *bytes = 0;
    if (!bytes || N < 1 || N > IMG_MAX_PLANES || n < 0 || n > SEL_MAX_N) return SPLATRASTER_ERR_BAD_ARG;
    *bytes = sel_layout(nullptr, N, n).total;
    return SPLATRASTER_OK;
}

int splatraster_masked_median(int32_t N, int64_t n, const float* values, int32_t positive_only, const float* opacity, float opacity_min,
                              const uint8_t* mask, float* median, float* std_out, int64_t* count, uint8_t* valid, void* workspace,
                              size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (N < 1 || N > IMG_MAX_PLANES || n < 0 || n > SEL_MAX_N || !median || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (n > 0 && !values) return SPLATRASTER_ERR_BAD_ARG;
    if (workspace_bytes < sel_layout(nullptr, N, n).total) return SPLATRASTER_ERR_BAD_ARG;
    return launch_frame_select(N, n, values, positive_only != 0, opacity, opacity_min, mask, median, std_out, count, valid, workspace,
                               stream);
}

}  // extern "C"
