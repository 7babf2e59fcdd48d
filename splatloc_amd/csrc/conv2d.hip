// conv2d.hip — the convolution layer both backbones are made of (SuperPoint's encoder and heads, NetVLAD's VGG16 trunk):
//   conv2d      3x3 (zero padding 1) or 1x1 cross-correlation, stride 1, + bias, ReLU, 2x2 / stride-2 max pool, as one implicit GEMM
//   preprocess  NetVLAD's input normalisation clamp(x * 255, 0, 255) - mean[c]
// The networks' definitions are not part of the reference tree: include/splatraster.h (splatraster_conv2d) and INTEGRATION.md §26
// hold the layer's contract, which is this project's own.
// Implicit GEMM on the exact-f32 MFMA (mfma_tile.h has its operand and accumulator layout): M = CV_CO output channels, N = a CV_ROWS x CV_COLS tile of output pixels, K = Cin k k walked
// in chunks of CV_CI input channels.  The im2col matrix never exists: a chunk's CV_CI planes of the pixel tile and its one-pixel
// halo (zero outside the image) and the matching weight slab are staged in LDS, and the taps are shifted reads of that patch.
// Determinism: no float atomics; every output is ONE fmaf chain from zero whose order is written down at the kernel and depends on
// (Cin, ksize) and the tile constants alone, then + bias.  Built with -ffp-contract=off.
#include "common.h"
#include "mfma_tile.h"

namespace sr {

namespace {

constexpr int CV_THREADS = 256;                       // four waves: wave w owns the tile's pixel rows 2 w and 2 w + 1
constexpr int CV_CO = 64;                             // output channels of a workgroup: two 32-row MFMA blocks
constexpr int CV_ROWS = 8, CV_COLS = 32;              // output pixels of a workgroup; a 32-pixel row is an MFMA's columns
constexpr int CV_CI = 8;                              // input channels staged per step
constexpr int CV_PROWS = CV_ROWS + 2, CV_PCOLS = CV_COLS + 2;   // the staged patch: the tile and its halo
constexpr int CV_PLD = CV_PCOLS;                      // row stride of a patch plane
constexpr int CV_PCH = CV_PROWS * CV_PLD + 12;        // plane stride: 352 = 32 mod 64, so an MFMA's two k planes read disjoint banks
constexpr int CV_PLANE = CV_PROWS * CV_PCOLS;         // staged elements of a plane
constexpr int CV_PLANE_PER_THREAD = (CV_PLANE + CV_THREADS - 1) / CV_THREADS;
constexpr int CV_WLD = 9 * CV_CI + 2;                 // row stride of the weight slab [co][tap * CV_CI + ci]: 74 = 10 mod 64 puts the 32
                                                      // rows of a block on the even banks and the second k (+ 1) on the odd ones
static_assert(CV_PCH % 64 == 32 && CV_WLD % 64 == 10 && CV_CI % 2 == 0, "bank layout of the two operands");
static_assert(CV_PLD == CV_PCOLS && CV_CO * 4 == CV_THREADS, "a plane is staged as it lies; four threads per weight row");
static_assert(CV_ROWS % 2 == 0 && CV_COLS % 2 == 0 && CV_ROWS == 2 * (CV_THREADS / WAVE), "pool windows never straddle a tile or a wave");

// One workgroup: image b, output channels [co0, co0 + CV_CO), output pixels [y0, y0 + CV_ROWS) x [x0, x0 + CV_COLS).
// THE CHAIN of out[b, co, y, x], with xp the zero-padded input and p = (KS - 1) / 2:
//     acc = 0
//     for c0 = 0, CV_CI, 2 CV_CI, ... < Cin:                          (chunks, ascending)
//       for ky = 0 .. KS - 1:  for kx = 0 .. KS - 1:                  (taps, row-major)
//         for ci = c0 .. c0 + CV_CI - 1:                              (channels of the chunk, ascending)
//           acc = fmaf(w[co, ci, ky, kx], xp[b, ci, y + ky - p, x + kx - p], acc)       (ci >= Cin: fmaf(0, 0, acc) = acc)
//     out = acc + bias[co];  ReLU: max(out, 0);  POOL2: the maximum of the 2x2 window
// A padded tap is fmaf(w, 0, acc) = acc: a border pixel follows the same statement.  Wave w accumulates [2 co blocks] x [pixel rows
// 2 w, 2 w + 1] as four independent 32x32 accumulators; an MFMA's two k are the channels ci, ci + 1 of one tap.  The pool's
// vertical maximum is between two accumulators of one lane, its horizontal one between neighbouring lanes.
template <int KS, bool VEC>
__global__ void __launch_bounds__(CV_THREADS)
conv2d_kernel(int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t cotiles, int32_t ytiles, int32_t xtiles,
              const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ bias, int32_t flags,
              float* __restrict__ out)
{
    constexpr int TAPS = KS * KS, P = (KS - 1) / 2;
    constexpr int WROW = TAPS * CV_CI;                          // staged weights of a chunk, per output channel
    constexpr int W_PER_THREAD = (WROW + 15) / 16 * 4;          // four threads per row, whole float4s
    __shared__ float s_x[CV_CI * CV_PCH];
    __shared__ float s_w[CV_CO * CV_WLD];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // neighbouring workgroups share an input patch (the channel tile runs fastest), then a row of the image
    uint32_t g = blockIdx.x;
    const int ct = g % cotiles; g /= cotiles;
    const int xt = g % xtiles; g /= xtiles;
    const int yt = g % ytiles; g /= ytiles;
    const int64_t b = g;
    const int co0 = ct * CV_CO, y0 = yt * CV_ROWS, x0 = xt * CV_COLS;
    const int32_t HW = H * W;                                   // Cin H W < 2^31: offsets inside one image fit 32 bits
    const float* xb = x + b * Cin * (int64_t)HW;

    // staged patch: plane ci of the chunk in round ci, element q = tid (+ CV_THREADS) of its CV_PROWS x CV_PCOLS pixels; the offset of
    // that pixel inside a plane is the same in every round (-1: outside the image or the patch)
    int32_t poff[CV_PLANE_PER_THREAD];
#pragma unroll
    for (int i = 0; i < CV_PLANE_PER_THREAD; ++i) {
        const int q = tid + CV_THREADS * i, yy = y0 - 1 + q / CV_PCOLS, xx = x0 - 1 + q % CV_PCOLS;
        poff[i] = (q < CV_PLANE && yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    float px[CV_CI][CV_PLANE_PER_THREAD], wv[W_PER_THREAD];
    // weight slab: thread (row co = tid / 4, quarter tid % 4) of the [CV_CO][CV_CI * TAPS] slab, a row being one run of memory; VEC: the
    // run as float4s (Cin a multiple of CV_CI, so no channel tail, and a 16-byte aligned base); zero beyond Cout and Cin
    const int wco = co0 + (tid >> 2), wq = tid & 3;
    auto fetch = [&](int c0) {
#pragma unroll
        for (int ci = 0; ci < CV_CI; ++ci) {
            const float* plane = xb + (int64_t)(c0 + ci) * HW;
            const bool live = c0 + ci < Cin;   // uniform
#pragma unroll
            for (int i = 0; i < CV_PLANE_PER_THREAD; ++i) px[ci][i] = (live && poff[i] >= 0) ? plane[poff[i]] : 0.f;
        }
        const float* wrow = weight + ((int64_t)wco * Cin + c0) * TAPS;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < W_PER_THREAD / 4; ++j) {
                const int f = wq + 4 * j;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (wco < Cout && 4 * f < WROW) t = *reinterpret_cast<const float4*>(wrow + 4 * f);
                wv[4 * j] = t.x, wv[4 * j + 1] = t.y, wv[4 * j + 2] = t.z, wv[4 * j + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < W_PER_THREAD; ++j) {
                const int r = 4 * (wq + 4 * (j >> 2)) + (j & 3);
                wv[j] = (wco < Cout && r < WROW && c0 + r / TAPS < Cin) ? wrow[r] : 0.f;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int ci = 0; ci < CV_CI; ++ci)
#pragma unroll
            for (int i = 0; i < CV_PLANE_PER_THREAD; ++i) {
                const int q = tid + CV_THREADS * i;
                if (q < CV_PLANE) s_x[ci * CV_PCH + q] = px[ci][i];   // CV_PLD == CV_PCOLS: a plane is stored as it is walked
            }
#pragma unroll
        for (int j = 0; j < W_PER_THREAD; ++j) {
            const int r = 4 * (wq + 4 * (j >> 2)) + (j & 3);
            if (r < WROW) s_w[(tid >> 2) * CV_WLD + (r % TAPS) * CV_CI + r / TAPS] = wv[j];
        }
    };

    f32x16 acc[2][2];   // [co block][pixel row of the wave]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc_zero(acc[m][n]);
    const bool two = co0 + 32 < Cout;   // the second block of channels exists (wave-uniform)
    const float* wa = s_w + c * CV_WLD + half;
    const float* xa = s_x + half * CV_PCH + (2 * wave + 1 - P) * CV_PLD + (1 - P) + c;
    fetch(0);
#pragma unroll 1
    for (int c0 = 0; c0 < Cin; c0 += CV_CI) {
        __syncthreads();   // the previous chunk's MFMAs have read the tiles
        stage();
        __syncthreads();
        if (c0 + CV_CI < Cin) fetch(c0 + CV_CI);   // in flight under the MFMAs
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int ky = t / KS, kx = t % KS;
#pragma unroll
            for (int s = 0; s < CV_CI / 2; ++s) {
                const float a0 = wa[t * CV_CI + 2 * s];
                const float b0 = xa[2 * s * CV_PCH + ky * CV_PLD + kx];
                const float b1 = xa[2 * s * CV_PCH + (ky + 1) * CV_PLD + kx];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                if (two) {
                    const float a1 = wa[32 * CV_WLD + t * CV_CI + 2 * s];
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                }
            }
        }
    }

    const bool relu = flags & SPLATRASTER_CONV_RELU;
    const int xx = x0 + c;
    if (flags & SPLATRASTER_CONV_POOL2) {
        const int Ho = H >> 1, Wo = W >> 1, yo = (y0 >> 1) + wave, xo = xx >> 1;
        float* ob = out + b * Cout * (int64_t)Ho * Wo;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + 32 * m + acc_row(i, half);
                const float bv = (bias && co < Cout) ? bias[co] : 0.f;
                float u = acc[m][0][i] + bv, v = acc[m][1][i] + bv;
                if (relu) u = fmaxf(u, 0.f), v = fmaxf(v, 0.f);
                u = fmaxf(u, v);
                u = fmaxf(u, __shfl_xor(u, 1, WAVE));   // every lane takes part
                if (!(c & 1) && co < Cout && yo < Ho && xo < Wo) ob[((int64_t)co * Ho + yo) * Wo + xo] = u;
            }
    } else {
        float* ob = out + b * Cout * (int64_t)HW;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int yy = y0 + 2 * wave + n;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int co = co0 + 32 * m + acc_row(i, half);
                    if (co < Cout && yy < H && xx < W) {
                        float v = bias ? acc[m][n][i] + bias[co] : acc[m][n][i];
                        if (relu) v = fmaxf(v, 0.f);
                        ob[((int64_t)co * H + yy) * W + xx] = v;
                    }
                }
            }
    }
}

constexpr int PP_THREADS = 256;

// out = clamp(x * 255, 0, 255) - mean[c]: three operations, each rounded on its own
__global__ void __launch_bounds__(PP_THREADS)
netvlad_preprocess_kernel(int64_t n, int32_t HW, const float* __restrict__ rgb, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int ch = (int)((i / HW) % 3);
    const float mean = ch == 0 ? 123.68f : ch == 1 ? 116.779f : 103.939f;
    out[i] = fminf(fmaxf(rgb[i] * 255.0f, 0.f), 255.0f) - mean;
}

constexpr int64_t CV_GRID_MAX = (1ll << 31) - 1;

struct CvPlan {
    int64_t cotiles, ytiles, xtiles, groups;
};

bool cv_shape_ok(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t flags, CvPlan* p)
{
    if (B < 0 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (ksize != 1 && ksize != 3)) return false;
    if (flags & ~(SPLATRASTER_CONV_RELU | SPLATRASTER_CONV_POOL2)) return false;
    if ((flags & SPLATRASTER_CONV_POOL2) && (H < 2 || W < 2)) return false;
    const int64_t hw = (int64_t)H * W;
    // a staged chunk reaches up to CV_CI - 1 planes past Cin before it is masked: those offsets fit 32 bits as well
    if (hw * Cin >= (1ll << 31) || hw * Cout >= (1ll << 31) || hw * CV_CI >= (1ll << 31)) return false;
    p->cotiles = ((int64_t)Cout + CV_CO - 1) / CV_CO;
    p->ytiles = ((int64_t)H + CV_ROWS - 1) / CV_ROWS;
    p->xtiles = ((int64_t)W + CV_COLS - 1) / CV_COLS;
    const int64_t per_image = p->cotiles * p->ytiles * p->xtiles;   // each count is at most its extent: <= Cout H W < 2^31
    if (per_image > CV_GRID_MAX || (B > 0 && per_image > CV_GRID_MAX / B)) return false;
    p->groups = per_image * B;
    return true;
}

bool cv_bad_ptr(const void* p) { return !p || misaligned(p, 4); }

}  // namespace

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_conv2d_tiles(int32_t* co_tile, int32_t* px_rows, int32_t* px_cols, int32_t* ci_chunk)
{
    if (!co_tile || !px_rows || !px_cols || !ci_chunk) return SPLATRASTER_ERR_BAD_ARG;
    *co_tile = CV_CO;
    *px_rows = CV_ROWS;
    *px_cols = CV_COLS;
    *ci_chunk = CV_CI;
    return SPLATRASTER_OK;
}

int splatraster_conv2d(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, const float* x, const float* weight,
                       const float* bias, int32_t flags, float* out, void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    (void)workspace_bytes;   // the layer needs none of it
    CvPlan p;
    if (!cv_shape_ok(B, Cin, Cout, H, W, ksize, flags, &p)) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (cv_bad_ptr(x) || cv_bad_ptr(weight) || cv_bad_ptr(out) || misaligned(bias, 4) || misaligned(workspace, 4)) return SPLATRASTER_ERR_BAD_ARG;
    // float4 weight loads where every chunk's run of a row is whole and 16-byte aligned, scalar loads otherwise: the same chain either way
    const bool vec = Cin % CV_CI == 0 && !misaligned(weight, 16);
    auto kernel = ksize == 3 ? (vec ? conv2d_kernel<3, true> : conv2d_kernel<3, false>) : (vec ? conv2d_kernel<1, true> : conv2d_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.groups), dim3(CV_THREADS), 0, stream, Cin, Cout, H, W, (int32_t)p.cotiles, (int32_t)p.ytiles,
                       (int32_t)p.xtiles, x, weight, bias, flags, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_netvlad_preprocess(int32_t B, int32_t H, int32_t W, const float* rgb, float* out, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (B < 0 || H < 1 || W < 1 || 3ll * H * W >= (1ll << 31)) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (cv_bad_ptr(rgb) || cv_bad_ptr(out)) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t n = 3ll * H * W * B, blocks = (n + PP_THREADS - 1) / PP_THREADS;
    if (blocks > CV_GRID_MAX) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(netvlad_preprocess_kernel, dim3((unsigned)blocks), dim3(PP_THREADS), 0, stream, n, H * W, rgb, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
