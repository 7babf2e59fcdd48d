// decoder.hip — SplatLoc's FeatureDecoder (models/decoders.py:43-68) and its training step (train_decoder.py:20-25,48-51,64-78)
// as fused kernels: bounding-box normalisation -> multiresolution grid encoding -> bias-free ReLU MLP -> unit normalisation, the
// cosine loss, the backward down to the weight and table gradients, and Adam over both parameter groups.
// Definition: include/splatraster.h (splatraster_decoder_layout) and INTEGRATION.md §19; design and measurements: DESIGN.md §18.
//
// Precision: f32 throughout.  Every matrix product runs on the exact f32-input MFMA v_mfma_f32_32x32x2_f32, whose result is a
// k-ordered fmaf chain: each dot product starts from a zero accumulator and adds its products with k ascending (mfma_tile.h has
// the operand and accumulator layout and the step of four k).
//
// Forward (decoder_fwd_kernel<D, F, RB>): one workgroup of 256 threads (4 waves) owns a tile of TM = 32 * RB points.
//   1. x is normalised with the bounding box in f64 ((x - lo) / (hi - lo), from the f64 or the exactly widened f32 input) and rounded
//      once to f32.
//   2. The grid encoding of grid_encoding.h goes straight into an LDS panel [TM][E + 4] (one (point, level) pair per thread and pass).
//   3. Layer l computes pre[p][o] = sum_k in[p][k] * W_l[o][k]: wave w owns the 32-column blocks w, w + 4, ... of the layer's
//      output, and for each keeps RB 32x32 accumulators (one per 32-point block) that share the B operand.  A comes from the LDS panel
//      (one 16-byte read per 4 k), B straight from global memory / L2 (lane (o, half) reads 16 bytes of row o of W_l per 4 k; the
//      272 KB of weights never fit LDS and every wave needs only its own rows).  ReLU in the epilogue; hidden activations ping-pong
//      between two LDS panels [TM][H + 4].
//   4. The last layer stays in registers (at most two column blocks per wave).  Sum of squares of a row, in this order: inside each
//      32-column block the squares are summed over the block's 32 lanes by an xor butterfly (lane distances 16, 8, 4, 2, 1); the
//      blocks' sums are then added in ascending column order starting from block 0.  out = f / sqrtf(sum) (a division; a zero row gives
//      0 / 0 = NaN as the reference does).
//   Inference writes out [N, O] only.  With `acts` the kernel also stores what the backward needs (decoder_acts_floats()).
//
// Backward (decoder_bwd_kernel): tiles of 32 points; workgroup g of G = min(tiles, DEC_BWD_MAX_WG) walks tiles g, g + G, ...
//   0. dL/df from dL/dout, or from the targets of the cosine loss (restated below), through the unit normalisation.
//   per layer, last to first: dW_l = dPre^T * H (sum over the tile's points, ascending) is added to the workgroup's own slab of the
//   workspace (plain read-modify-write by the one thread that owns the element: no atomics), dH = dPre * W_l (sum over o ascending)
//   is masked with the stored activation (> 0) and becomes the next dPre; layer 0's dH is dL/d(encoded), written to the workspace.
//   decoder_reduce_kernel then sums the G slabs in ascending g (bit-reproducible weight gradients) and the tiles' loss terms in a
//   fixed order; the table gradient is the arrival-ordered scatter of grid_encoding.hip, run as the next launch.
//
// Cosine loss (train_decoder.py:23-25, torch.cosine_similarity with eps 1e-8): cos_i = (y_i . t_i) / (max(|y_i|, eps) max(|t_i|, eps)),
// loss = 1 - (sum_i cos_i) / N.  Each dot product is 8 ascending partial chains of O / 8 columns combined by an xor butterfly
// (1, 2, 4); a tile's cosines are summed in row order, the tiles by decoder_reduce_kernel (256 strided ascending chains, then a
// binary tree).
//
// Adam (decoder_adam_kernel): torch.optim.Adam of the two groups in one launch, dense over the table; the pass that reads a gradient
// writes it back as zero.
//
// LDS per workgroup / occupancy designed for (pinned by tests/test_decoder_codegen.py): forward RB = 2: 70 656 B, RB = 1: 35 328 B;
// backward 67 200 B; two workgroups (8 waves) per CU, i.e. 2 waves per SIMD, at most 256 VGPRs, no scratch.
#include "common.h"
#include "grid_encoding.h"
#include "mfma_tile.h"

#include <math.h>

namespace sr {

constexpr int DEC_THREADS = 256;
constexpr int DEC_MAX_H = 128;     // hidden width (and encoded width) the panels are sized for
constexpr int DEC_MAX_O = 256;     // output width
constexpr int DEC_PAD = 4;         // floats of padding per panel row (keeps rows 16-byte aligned, spreads the banks)
constexpr int DEC_BWD_TM = 32;
constexpr int DEC_BWD_MAX_WG = 64;
constexpr int DEC_MAX_LAYERS = SPLATRASTER_DECODER_MAX_LAYERS;

struct DecArgs {
    double lo[3], hi[3];
    int32_t n_layers;
    int32_t dims[DEC_MAX_LAYERS + 1];
    int64_t woff[DEC_MAX_LAYERS + 1];   // float offset of layer l in the flat weight-gradient vector; woff[n_layers] = total
    int32_t x_f64;                      // the points are f64
};

// the backward's view of DecArgs: no bounding box, 32-bit offsets (fewer scalar registers held across the layer loop)
struct DecBwdArgs {
    int32_t n_layers;
    int32_t dims[DEC_MAX_LAYERS + 1];
    int32_t woff[DEC_MAX_LAYERS + 1];
};

struct DecWeights {
    const float* w[DEC_MAX_LAYERS];
};

// ---- activation record of the training forward (floats) ---------------------------------------------------------------
// [enc N x E][h_1 N x H] ... [h_{n-1} N x H][f N x O (unnormalised)][norm N][xn N x D (normalised points, f32)]
template <class A>
__host__ __device__ static inline int64_t acts_layer_offset(const A& d, int64_t N, int l)   // input of layer l; l == n_layers: f
{
    int64_t off = 0;
    for (int i = 0; i < l; ++i) off += N * d.dims[i];
    return off;
}
template <class A>
__host__ __device__ static inline int64_t acts_norm_offset(const A& d, int64_t N)
{
    return acts_layer_offset(d, N, d.n_layers) + N * d.dims[d.n_layers];
}
template <class A>
__host__ __device__ static inline int64_t acts_xn_offset(const A& d, int64_t N) { return acts_norm_offset(d, N) + N; }

// the value in a vector register the optimiser cannot see through: epilogue addresses built from it are computed per lane where they
// are used, not hoisted out of the block loops as dozens of long-lived scalar registers
__device__ __forceinline__ int in_vgpr(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float butterfly32(float v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// acc[rb] += in[rb * 32 + c][k] * wrow[k] for k = 0 .. K - 1 ascending (c = lane & 31; wrow = the lane's own row of W)
template <int RB>
__device__ __forceinline__ void layer_block(f32x16 (&acc)[RB], const float* in, int ld_in, const float* __restrict__ wrow, int K,
                                            int c, int half)
{
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 16) {
        float4 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(wrow + k0 + 4 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 bj = pick(b[j], half);   // once per j: every block of the tile shares it
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                mfma_k4(acc[rb], pick(*reinterpret_cast<const float4*>(in + (rb * 32 + c) * ld_in + k0 + 4 * j), half), bj);
        }
    }
}

template <int D, int F, int RB>
__global__ void __launch_bounds__(DEC_THREADS)
decoder_fwd_kernel(int64_t N, GridArgs a, DecArgs d, const void* __restrict__ x, const float* __restrict__ table, DecWeights W,
                   float* __restrict__ out, float* __restrict__ acts)
{
    constexpr int TM = 32 * RB;
    constexpr int LD = DEC_MAX_H + DEC_PAD;
    __shared__ __attribute__((aligned(16))) float s_panel[2][TM * LD];
    __shared__ float s_ssq[TM][DEC_MAX_O / 32];
    __shared__ float s_x[TM][4];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the block loops below are scalar loops
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    const int E = d.dims[0];
    const int n_live = (int)(N - row0 < TM ? N - row0 : TM);   // rows of the tile that are points

    // 1. normalise (f64, one rounding to f32)
    if (tid < TM * D) {
        const int r = tid / D, k = tid - r * D;
        const int64_t n = row0 + r;
        float v = 0.f;
        if (n < N) {
            const double xv = d.x_f64 ? static_cast<const double*>(x)[n * D + k] : (double)static_cast<const float*>(x)[n * D + k];
            v = (float)((xv - d.lo[k]) / (d.hi[k] - d.lo[k]));
            if (acts) acts[acts_xn_offset(d, N) + n * D + k] = v;
        }
        s_x[r][k] = v;
    }
    __syncthreads();

    // 2. encode into panel 0 (rows past N: zeros)
    {
        const int ld = E + DEC_PAD;
        for (int t = tid; t < (TM << a.lp_log2); t += DEC_THREADS) {
            const int r = t >> a.lp_log2, level = t & ((1 << a.lp_log2) - 1);
            if (level >= a.n_levels) continue;
            const int64_t n = row0 + r;
            float acc[F];
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = 0.f;
            if (n < N) {
                const Locus<D> q = locate<D>(a.scale[level], s_x[r]);
                const uint32_t res = a.res[level], size = a.size[level];
                const float* grid = table + (size_t)a.offset[level] * F;
                constexpr int C = 1 << D;
                Feat<F> v[C];
#pragma unroll
                for (int cc = 0; cc < C; ++cc) v[cc] = load_feat<F>(grid + (size_t)corner_index<D>(q, cc, res, size, a.hashed) * F);
#pragma unroll
                for (int cc = 0; cc < C; ++cc) {
                    const float w = corner_weight<D>(q, cc);
#pragma unroll
                    for (int f = 0; f < F; ++f) acc[f] = fmaf(w, v[cc].v[f], acc[f]);
                }
                if (acts) store_feat<F>(acts + n * (int64_t)E + level * F, acc);
            }
#pragma unroll
            for (int f = 0; f < F; ++f) s_panel[0][r * ld + level * F + f] = acc[f];
        }
    }
    __syncthreads();

    // 3. hidden layers
    const int nl = d.n_layers;
    int cur = 0;
    for (int l = 0; l + 1 < nl; ++l) {
        const int K = d.dims[l], No = d.dims[l + 1];
        const float* in = s_panel[cur];
        float* nxt = s_panel[cur ^ 1];
        const int ld_in = K + DEC_PAD, ld_out = No + DEC_PAD;
        float* h_out = acts ? acts + acts_layer_offset(d, N, l + 1) : nullptr;
        for (int cb = wave; cb < (No >> 5); cb += 4) {
            f32x16 acc[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc_zero(acc[rb]);
            layer_block<RB>(acc, in, ld_in, W.w[l] + (size_t)(cb * 32 + c) * K, K, c, half);
            const int ldv = in_vgpr(ld_out), nov = in_vgpr(No), live = in_vgpr(h_out ? n_live : 0);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int r = rb * 32 + acc_row(i, half);
                    const float v = fmaxf(acc[rb][i], 0.f);
                    nxt[r * ldv + cb * 32 + c] = v;
                    if (r < live) h_out[(row0 + r) * nov + cb * 32 + c] = v;
                }
        }
        __syncthreads();
        cur ^= 1;
    }

    // 4. last layer in registers, unit normalisation
    {
        const int K = d.dims[nl - 1], O = d.dims[nl];
        const float* in = s_panel[cur];
        const int ld_in = K + DEC_PAD, ncb = O >> 5;
        f32x16 acc[2][RB];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // element by element, not acc_zero(): zeroed as whole vectors, these 2 RB accumulators that live across the barrier give the
            // forward another register assignment and schedule throughout; this form keeps its instructions as they were (HISTORY.md §35)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[s][rb][i] = 0.f;
            const int cb = wave + 4 * s;
            if (cb < ncb) {
                layer_block<RB>(acc[s], in, ld_in, W.w[nl - 1] + (size_t)(cb * 32 + c) * K, K, c, half);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float q = butterfly32(acc[s][rb][i] * acc[s][rb][i]);
                        if (c == 0) s_ssq[rb * 32 + acc_row(i, half)][cb] = q;
                    }
            }
        }
        __syncthreads();
        float* f_out = acts ? acts + acts_layer_offset(d, N, nl) : nullptr;
        float* n_out = acts ? acts + acts_norm_offset(d, N) : nullptr;
        const int ov = in_vgpr(O);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = rb * 32 + acc_row(i, half);
                float ss = s_ssq[r][0];
                for (int b = 1; b < ncb; ++b) ss += s_ssq[r][b];
                const float nrm = sqrtf(ss);
                const int64_t n = row0 + r;
                if (r < n_live) {
                    if (n_out && wave == 0 && c == 0) n_out[n] = nrm;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int cb = wave + 4 * s;
                        if (cb < ncb) {
                            out[n * ov + cb * 32 + c] = acc[s][rb][i] / nrm;
                            if (f_out) f_out[n * ov + cb * 32 + c] = acc[s][rb][i];
                        }
                    }
                }
            }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DEC_THREADS)
decoder_bwd_kernel(int64_t N, int32_t n_tiles, DecBwdArgs d, DecWeights W, const float* __restrict__ acts,
                   const float* __restrict__ dL_dout, const float* __restrict__ targets, float inv_N, float* __restrict__ slabs,
                   float* __restrict__ loss_part, float* __restrict__ denc)
{
    constexpr int TM = DEC_BWD_TM;
    constexpr int LDA = DEC_MAX_O + DEC_PAD, LDB = DEC_MAX_H + DEC_PAD;
    __shared__ __attribute__((aligned(16))) float s_ga[TM * LDA];   // dPre of the last layer, then every second one below
    __shared__ __attribute__((aligned(16))) float s_gb[TM * LDB];   // the dPre panels in between
    __shared__ __attribute__((aligned(16))) float s_h[TM * LDB];    // input activation of the layer
    __shared__ float s_cos[TM];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the block loops below are scalar loops
    const int nl = d.n_layers, O = d.dims[nl];
    float* slab = slabs + (size_t)blockIdx.x * d.woff[nl];
    const float eps = 1e-8f;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int64_t row0 = (int64_t)tile * TM;
        const int n_live = (int)(N - row0 < TM ? N - row0 : TM);

        // 0. dL/df of the tile -> s_ga: 8 threads per row, O / 8 contiguous columns each
        {
            const int r = tid >> 3, q = tid & 7, w = O >> 3;
            const int64_t n = row0 + r;
            const bool live = n < N;
            const float* f = acts + acts_layer_offset(d, N, nl) + (live ? n : 0) * O + q * w;
            const float nrm = acts[acts_norm_offset(d, N) + (live ? n : 0)];
            const float* g = (targets ? targets : dL_dout) + (live ? n : 0) * O + q * w;
            float yg = 0.f, yy = 0.f, gg = 0.f;
            for (int k = 0; k < w; k += 4) {
                const float4 fv = *reinterpret_cast<const float4*>(f + k), gv = *reinterpret_cast<const float4*>(g + k);
                const float y0 = fv.x / nrm, y1 = fv.y / nrm, y2 = fv.z / nrm, y3 = fv.w / nrm;
                yg = fmaf(y0, gv.x, yg); yg = fmaf(y1, gv.y, yg); yg = fmaf(y2, gv.z, yg); yg = fmaf(y3, gv.w, yg);
                yy = fmaf(y0, y0, yy); yy = fmaf(y1, y1, yy); yy = fmaf(y2, y2, yy); yy = fmaf(y3, y3, yy);
                gg = fmaf(gv.x, gv.x, gg); gg = fmaf(gv.y, gv.y, gg); gg = fmaf(gv.z, gv.z, gg); gg = fmaf(gv.w, gv.w, gg);
            }
#pragma unroll
            for (int m = 1; m <= 4; m <<= 1) {
                yg += __shfl_xor(yg, m);
                yy += __shfl_xor(yy, m);
                gg += __shfl_xor(gg, m);
            }
            // dL/dy = ca * g + cb * y;  s = y . dL/dy;  dL/df = (dL/dy - y s) / |f|
            float ca = 1.f, cb = 0.f;
            if (targets) {
                const float ny = sqrtf(yy), nt = sqrtf(gg);
                const float cy = fmaxf(ny, eps), ct = fmaxf(nt, eps);
                const float ia = 1.f / (cy * ct);
                const float cosv = yg * ia;
                if (q == 0) s_cos[r] = live ? cosv : 0.f;
                ca = -inv_N * ia;
                cb = ny > eps ? inv_N * (cosv / (cy * ny)) : 0.f;
            }
            const float s = ca * yg + cb * yy;
            for (int k = 0; k < w; k += 4) {
                const float4 fv = *reinterpret_cast<const float4*>(f + k), gv = *reinterpret_cast<const float4*>(g + k);
                float4 o;
                float y;
                y = fv.x / nrm; o.x = ((ca * gv.x + cb * y) - y * s) / nrm;
                y = fv.y / nrm; o.y = ((ca * gv.y + cb * y) - y * s) / nrm;
                y = fv.z / nrm; o.z = ((ca * gv.z + cb * y) - y * s) / nrm;
                y = fv.w / nrm; o.w = ((ca * gv.w + cb * y) - y * s) / nrm;
                if (!live) o = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(s_ga + r * (O + DEC_PAD) + q * w + k) = o;
            }
        }
        __syncthreads();
        if (targets && tid == 0) {
            float sum = 0.f;
            for (int r = 0; r < TM; ++r) sum += s_cos[r];
            loss_part[tile] = sum;
        }

        float* cur = s_ga;
        float* nxt = s_gb;
#pragma unroll 1
        for (int l = nl - 1; l >= 0; --l) {
            const int K = d.dims[l], No = d.dims[l + 1];
            const int ldp = No + DEC_PAD, ldh = K + DEC_PAD;
            // input activation of the layer -> s_h (rows past N: zeros)
            {
                const float* h = acts + acts_layer_offset(d, N, l);
                const int kq = K >> 2;
                for (int t = tid; t < TM * kq; t += DEC_THREADS) {
                    const int r = t / kq, k = (t - r * kq) * 4;
                    const int64_t n = row0 + r;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (n < N) v = *reinterpret_cast<const float4*>(h + n * K + k);
                    *reinterpret_cast<float4*>(s_h + r * ldh + k) = v;
                }
            }
            __syncthreads();
            const int nkb = (K + 31) >> 5, nob = No >> 5;
            // dW_l[o][k] = sum_p dPre[p][o] * H[p][k], p ascending
            float* wslab = slab + d.woff[l];
#pragma unroll 1
            for (int b = wave; b < nob * nkb; b += 4) {
                const int ob = b / nkb, kb = b - ob * nkb;
                const bool kval = kb * 32 + c < K;
                f32x16 acc;
                acc_zero(acc);
#pragma unroll 4
                for (int p = 0; p < TM; p += 2) {
                    const float av = cur[(p + half) * ldp + ob * 32 + c];
                    const float hv = s_h[(p + half) * ldh + kb * 32 + c];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, kval ? hv : 0.f, acc, 0, 0, 0);
                }
                if (kval) {
                    const int kv = in_vgpr(K);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        float* p = wslab + (size_t)((ob * 32 + acc_row(i, half)) * kv) + kb * 32 + c;
                        *p = first ? acc[i] : *p + acc[i];
                    }
                }
            }
            // dH[p][k] = sum_o dPre[p][o] * W_l[o][k], o ascending; masked with the activation; layer 0: dL/d(encoded)
#pragma unroll 1
            for (int kb = wave; kb < nkb; kb += 4) {
                const bool kval = kb * 32 + c < K;
                const float* wcol = W.w[l] + kb * 32 + (kval ? c : 0);
                f32x16 acc;
                acc_zero(acc);
#pragma unroll 2
                for (int o0 = 0; o0 < No; o0 += 4) {
                    const float b0 = wcol[(size_t)(o0 + half) * K], b1 = wcol[(size_t)(o0 + 2 + half) * K];
                    mfma_k4(acc, pick(*reinterpret_cast<const float4*>(cur + c * ldp + o0), half), make_float2(kval ? b0 : 0.f, kval ? b1 : 0.f));
                }
                if (kval) {
                    const int ldv = in_vgpr(ldh), kv = in_vgpr(K), live = in_vgpr(n_live);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int r = acc_row(i, half);
                        if (l > 0) {
                            nxt[r * ldv + kb * 32 + c] = s_h[r * ldv + kb * 32 + c] > 0.f ? acc[i] : 0.f;
                        } else if (r < live) {
                            denc[(row0 + r) * kv + kb * 32 + c] = acc[i];
                        }
                    }
                }
            }
            __syncthreads();
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
    }
}

// dW[i] = sum over the G slabs, ascending; block 0 also reduces the tiles' cosine sums: loss = 1 - sum / N
__global__ void __launch_bounds__(DEC_THREADS)
decoder_reduce_kernel(int64_t n_w, int32_t G, const float* __restrict__ slabs, float* __restrict__ dW, int32_t n_tiles,
                      const float* __restrict__ loss_part, float inv_N, float* __restrict__ loss)
{
    __shared__ float s_red[DEC_THREADS];
    for (int64_t i = (int64_t)blockIdx.x * DEC_THREADS + threadIdx.x; i < n_w; i += (int64_t)gridDim.x * DEC_THREADS) {
        float s = slabs[i];
        for (int g = 1; g < G; ++g) s += slabs[(size_t)g * n_w + i];
        dW[i] = s;
    }
    if (blockIdx.x == 0 && loss) {
        float s = 0.f;
        for (int t = threadIdx.x; t < n_tiles; t += DEC_THREADS) s += loss_part[t];
        s_red[threadIdx.x] = s;
        __syncthreads();
        for (int m = DEC_THREADS / 2; m >= 1; m >>= 1) {
            if ((int)threadIdx.x < m) s_red[threadIdx.x] += s_red[threadIdx.x + m];
            __syncthreads();
        }
        if (threadIdx.x == 0) loss[0] = 1.f - s_red[0] * inv_N;
    }
}

// ---- Adam over both groups ----------------------------------------------------------------------------------------------
struct DecAdam {
    float* w[DEC_MAX_LAYERS];
    int64_t woff[DEC_MAX_LAYERS + 1];
    int32_t n_layers;
    float *w_grad, *w_m, *w_v;           // flat [woff[n_layers]]
    float *table, *t_grad, *t_m, *t_v;   // [n_table]
    int64_t n_table;
    float omb1, beta2, omb2;
    float step_w, step_t;                // lr / (1 - beta1^t)
    float bc2_sqrt;                      // sqrt(1 - beta2^t)
    float eps_w, eps_t, weight_decay;
};

// torch.optim.Adam (its foreach form), with the roundings of torch's own elementwise kernels: every foreach op is one kernel whose
// lambda hipcc contracts, so  g += wd p  is fma(wd, p, g);  exp_avg.lerp_(g, 1 - beta1)  is fma(1 - beta1, g - m, m);
// exp_avg_sq.mul_(beta2)  rounds on its own and  .addcmul_(g, g, 1 - beta2)  is fma(1 - beta2, g g, .);
// denom = sqrt(v) / sqrt(1 - beta2^t) + eps  is three roundings;  p.addcdiv_(m, denom, -lr / (1 - beta1^t))  is fma(-step, m / denom, p).
// Written with explicit fmaf under contract(off) so that nothing else fuses.
__device__ __forceinline__ void dec_adam_element(const DecAdam& A, float g, float& m, float& v, float& p, float step, float eps)
{
#pragma clang fp contract(off)
    m = __builtin_fmaf(A.omb1, g - m, m);
    const float gg = g * g;
    const float vb = v * A.beta2;
    v = __builtin_fmaf(A.omb2, gg, vb);
    const float denom = sqrtf(v) / A.bc2_sqrt + eps;
    p = __builtin_fmaf(-step, m / denom, p);
}

__global__ void __launch_bounds__(DEC_THREADS)
decoder_adam_kernel(DecAdam A)
{
    const int64_t quads = A.n_table >> 2, n_w = A.woff[A.n_layers];
    const int64_t total = quads + (A.n_table & 3) + n_w;
    for (int64_t e = (int64_t)blockIdx.x * DEC_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DEC_THREADS) {
        if (e < quads) {
            float4 g = reinterpret_cast<float4*>(A.t_grad)[e];
            float4 m = reinterpret_cast<float4*>(A.t_m)[e], v = reinterpret_cast<float4*>(A.t_v)[e];
            float4 p = reinterpret_cast<float4*>(A.table)[e];
            dec_adam_element(A, g.x, m.x, v.x, p.x, A.step_t, A.eps_t);
            dec_adam_element(A, g.y, m.y, v.y, p.y, A.step_t, A.eps_t);
            dec_adam_element(A, g.z, m.z, v.z, p.z, A.step_t, A.eps_t);
            dec_adam_element(A, g.w, m.w, v.w, p.w, A.step_t, A.eps_t);
            reinterpret_cast<float4*>(A.t_m)[e] = m;
            reinterpret_cast<float4*>(A.t_v)[e] = v;
            reinterpret_cast<float4*>(A.table)[e] = p;
            reinterpret_cast<float4*>(A.t_grad)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (e < quads + (A.n_table & 3)) {
            const int64_t k = (quads << 2) + (e - quads);
            float m = A.t_m[k], v = A.t_v[k], p = A.table[k];
            dec_adam_element(A, A.t_grad[k], m, v, p, A.step_t, A.eps_t);
            A.t_m[k] = m; A.t_v[k] = v; A.table[k] = p; A.t_grad[k] = 0.f;
        } else {
            const int64_t k = e - quads - (A.n_table & 3);
            int l = 0;
#pragma unroll 1
            while (l + 1 < A.n_layers && k >= A.woff[l + 1]) ++l;
            float* pp = A.w[l] + (k - A.woff[l]);
            float m = A.w_m[k], v = A.w_v[k], p = *pp;
            const float g = __builtin_fmaf(A.weight_decay, p, A.w_grad[k]);
            dec_adam_element(A, g, m, v, p, A.step_w, A.eps_w);
            A.w_m[k] = m; A.w_v[k] = v; *pp = p; A.w_grad[k] = 0.f;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static int dec_args(const splatraster_decoder_layout* lay, GridArgs* a, DecArgs* d)
{
    if (!lay) return SPLATRASTER_ERR_BAD_ARG;
    const int st = grid_args(&lay->grid, a);
    if (st) return st == SPLATRASTER_ERR_UNSUPPORTED ? SPLATRASTER_ERR_BAD_ARG : st;
    const int D = lay->grid.n_dims, E = lay->grid.n_levels * lay->grid.n_features, nl = lay->n_layers;
    if (nl < 2 || nl > DEC_MAX_LAYERS) return SPLATRASTER_ERR_BAD_ARG;
    if (E % 16 != 0 || E > 64 || lay->dims[0] != E) return SPLATRASTER_ERR_BAD_ARG;
    const int H = lay->dims[1], O = lay->dims[nl];
    if (H != 32 && H != 64 && H != 128) return SPLATRASTER_ERR_BAD_ARG;
    for (int l = 1; l < nl; ++l)
        if (lay->dims[l] != H) return SPLATRASTER_ERR_BAD_ARG;
    if (O < 32 || O > DEC_MAX_O || O % 32 != 0) return SPLATRASTER_ERR_BAD_ARG;
    memset(d, 0, sizeof(*d));
    for (int k = 0; k < D; ++k) {
        d->lo[k] = lay->bound[k][0];
        d->hi[k] = lay->bound[k][1];
        if (!isfinite(d->lo[k]) || !isfinite(d->hi[k])) return SPLATRASTER_ERR_BAD_ARG;
    }
    d->n_layers = nl;
    int64_t off = 0;
    for (int l = 0; l <= nl; ++l) {
        d->dims[l] = lay->dims[l];
        d->woff[l] = off;
        if (l < nl) off += (int64_t)lay->dims[l] * lay->dims[l + 1];
    }
    return SPLATRASTER_OK;
}

static int64_t dec_acts_floats(const DecArgs& d, int64_t N, int D) { return acts_xn_offset(d, N) + N * D; }
static int dec_bwd_tiles(int64_t N) { return (int)((N + DEC_BWD_TM - 1) / DEC_BWD_TM); }
static int dec_bwd_groups(int64_t N) { const int t = dec_bwd_tiles(N); return t < DEC_BWD_MAX_WG ? t : DEC_BWD_MAX_WG; }
// tiles of every launch fit an int and the activation record stays addressable
static bool dec_n_ok(int64_t N) { return N >= 0 && N <= (int64_t(1) << 30); }

struct DecWorkspace {
    float *slabs, *loss_part, *denc;
    size_t total;
};
static DecWorkspace dec_workspace(void* base, const DecArgs& d, int64_t N)
{
    DecWorkspace w;
    Carver c{base};
    w.slabs = c.take<float>((size_t)dec_bwd_groups(N) * d.woff[d.n_layers]);
    w.loss_part = c.take<float>((size_t)dec_bwd_tiles(N));
    w.denc = c.take<float>((size_t)N * d.dims[0]);
    w.total = c.o;
    return w;
}

static int dec_weights(const DecArgs& d, const float* const* weights, DecWeights* W)
{
    if (!weights) return SPLATRASTER_ERR_BAD_ARG;
    for (int l = 0; l < DEC_MAX_LAYERS; ++l) {
        W->w[l] = l < d.n_layers ? weights[l] : nullptr;
        if (l < d.n_layers && (!W->w[l] || misaligned(W->w[l], 16))) return SPLATRASTER_ERR_BAD_ARG;
    }
    return SPLATRASTER_OK;
}

template <int D, int F>
static void launch_dec_fwd(int64_t N, const GridArgs& a, const DecArgs& d, const void* x, const float* table, const DecWeights& W,
                           float* out, float* acts, hipStream_t s)
{
    // 64-point tiles once they fill the machine twice over; 32-point tiles below that (more workgroups for a small batch).
    // Both give the same bits: an output element is the same k-ordered chain whatever the tile height.
    if (N >= 64 * 512) {
        hipLaunchKernelGGL((decoder_fwd_kernel<D, F, 2>), dim3((unsigned)((N + 63) / 64)), dim3(DEC_THREADS), 0, s, N, a, d, x, table,
                           W, out, acts);
    } else {
        hipLaunchKernelGGL((decoder_fwd_kernel<D, F, 1>), dim3((unsigned)((N + 31) / 32)), dim3(DEC_THREADS), 0, s, N, a, d, x, table,
                           W, out, acts);
    }
}

#define SR_DEC_DISPATCH(D, F, CALL)                            \
    do {                                                       \
        switch ((D) * 16 + (F)) {                              \
        case 2 * 16 + 1: CALL(2, 1); break;                    \
        case 2 * 16 + 2: CALL(2, 2); break;                    \
        case 2 * 16 + 4: CALL(2, 4); break;                    \
        case 2 * 16 + 8: CALL(2, 8); break;                    \
        case 3 * 16 + 1: CALL(3, 1); break;                    \
        case 3 * 16 + 2: CALL(3, 2); break;                    \
        case 3 * 16 + 4: CALL(3, 4); break;                    \
        case 3 * 16 + 8: CALL(3, 8); break;                    \
        default: return SPLATRASTER_ERR_BAD_ARG;               \
        }                                                      \
    } while (0)

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_decoder_workspace_bytes(const splatraster_decoder_layout* lay, int64_t N, size_t* workspace_bytes,
                                        size_t* activation_bytes)
{
    GridArgs a;
    DecArgs d;
    const int st = dec_args(lay, &a, &d);
    if (st) return st;
    if (!dec_n_ok(N)) return SPLATRASTER_ERR_BAD_ARG;
    if (workspace_bytes) *workspace_bytes = dec_workspace(nullptr, d, N).total;
    if (activation_bytes) *activation_bytes = (size_t)dec_acts_floats(d, N, lay->grid.n_dims) * sizeof(float);
    return SPLATRASTER_OK;
}

int splatraster_decoder_forward(const splatraster_decoder_layout* lay, int64_t N, const void* x, int32_t x_is_f64,
                                const float* table, const float* const* weights, float* out, float* acts, void* stream)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GridArgs a;
    DecArgs d;
    int st = dec_args(lay, &a, &d);
    if (st) return st;
    DecWeights W;
    st = dec_weights(d, weights, &W);
    if (st) return st;
    if (!dec_n_ok(N)) return SPLATRASTER_ERR_BAD_ARG;
    if (N == 0) return SPLATRASTER_OK;
    if (!x || !table || !out || misaligned(table, 16) || misaligned(out, 16) || misaligned(acts, 16) ||
        (reinterpret_cast<uintptr_t>(x) & (x_is_f64 ? 7u : 3u)))
        return SPLATRASTER_ERR_BAD_ARG;
    d.x_f64 = x_is_f64 != 0;
#define SR_CALL(dd, ff) launch_dec_fwd<dd, ff>(N, a, d, x, table, W, out, acts, s)
    SR_DEC_DISPATCH(lay->grid.n_dims, lay->grid.n_features, SR_CALL);
#undef SR_CALL
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_decoder_backward(const splatraster_decoder_layout* lay, int64_t N, const float* table,
                                 const float* const* weights, const float* acts, const float* dL_dout, const float* targets,
                                 float* loss, float* dL_dweights, float* dL_dtable, float* dL_dx, void* workspace, void* stream)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GridArgs a;
    DecArgs d;
    int st = dec_args(lay, &a, &d);
    if (st) return st;
    DecWeights W;
    st = dec_weights(d, weights, &W);
    if (st) return st;
    if (!dec_n_ok(N)) return SPLATRASTER_ERR_BAD_ARG;
    if ((dL_dout == nullptr) == (targets == nullptr)) return SPLATRASTER_ERR_BAD_ARG;   // exactly one of the two
    if (loss && !targets) return SPLATRASTER_ERR_BAD_ARG;
    if (N == 0) return SPLATRASTER_ERR_BAD_ARG;            // an empty batch has no mean; the caller returns zero gradients
    if (!acts || !dL_dweights || !workspace || misaligned(acts, 16) || misaligned(dL_dout, 16) || misaligned(targets, 16) ||
        misaligned(dL_dweights, 16) || misaligned(dL_dtable, 16) || misaligned(workspace, 16) || (dL_dx && (!table || misaligned(table, 16))))
        return SPLATRASTER_ERR_BAD_ARG;
    const DecWorkspace w = dec_workspace(workspace, d, N);
    float *slabs = w.slabs, *loss_part = w.loss_part, *denc = w.denc;
    const int tiles = dec_bwd_tiles(N), G = dec_bwd_groups(N);
    const float inv_N = 1.0f / (float)N;
    DecBwdArgs bd{};
    bd.n_layers = d.n_layers;
    for (int l = 0; l <= d.n_layers; ++l) {
        bd.dims[l] = d.dims[l];
        bd.woff[l] = (int32_t)d.woff[l];
    }
    hipLaunchKernelGGL(decoder_bwd_kernel, dim3(G), dim3(DEC_THREADS), 0, s, N, tiles, bd, W, acts, dL_dout, targets, inv_N, slabs,
                       loss_part, denc);
    SR_LAUNCH_CHECK();
    const int64_t n_w = d.woff[d.n_layers];
    hipLaunchKernelGGL(decoder_reduce_kernel, dim3((unsigned)((n_w + DEC_THREADS - 1) / DEC_THREADS)), dim3(DEC_THREADS), 0, s, n_w,
                       G, slabs, dL_dweights, tiles, loss_part, inv_N, targets ? loss : nullptr);
    SR_LAUNCH_CHECK();
    if (dL_dtable || dL_dx)
        return splatraster_grid_encoding_backward(&lay->grid, N, acts + acts_xn_offset(d, N), table, denc, dL_dtable, dL_dx, stream);
    return SPLATRASTER_OK;
}

int splatraster_decoder_adam(const splatraster_decoder_layout* lay, float* const* weights, float* w_grad, float* w_m, float* w_v,
                             float* table, float* t_grad, float* t_m, float* t_v, int64_t step, double lr_w, double lr_t,
                             double beta1, double beta2, double eps_w, double eps_t, double weight_decay, void* stream)
{
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GridArgs a;
    DecArgs d;
    int st = dec_args(lay, &a, &d);
    if (st) return st;
    DecWeights W;
    st = dec_weights(d, weights, &W);
    if (st) return st;
    if (step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return SPLATRASTER_ERR_BAD_ARG;
    if (!w_grad || !w_m || !w_v || !table || !t_grad || !t_m || !t_v || misaligned(table, 16) || misaligned(t_grad, 16) || misaligned(t_m, 16) ||
        misaligned(t_v, 16))
        return SPLATRASTER_ERR_BAD_ARG;
    DecAdam A{};
    for (int l = 0; l < d.n_layers; ++l) A.w[l] = weights[l];
    for (int l = 0; l <= d.n_layers; ++l) A.woff[l] = d.woff[l];
    A.n_layers = d.n_layers;
    A.w_grad = w_grad; A.w_m = w_m; A.w_v = w_v;
    A.table = table; A.t_grad = t_grad; A.t_m = t_m; A.t_v = t_v;
    A.n_table = lay->grid.n_params;
    A.omb1 = (float)(1.0 - beta1);
    A.beta2 = (float)beta2;
    A.omb2 = (float)(1.0 - beta2);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    A.step_w = (float)(lr_w / bc1);
    A.step_t = (float)(lr_t / bc1);
    A.bc2_sqrt = (float)sqrt(bc2);
    A.eps_w = (float)eps_w;
    A.eps_t = (float)eps_t;
    A.weight_decay = (float)weight_decay;
    const int64_t total = (A.n_table >> 2) + (A.n_table & 3) + d.woff[d.n_layers];
    int64_t blocks = (total + DEC_THREADS - 1) / DEC_THREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(decoder_adam_kernel, dim3((unsigned)blocks), dim3(DEC_THREADS), 0, s, A);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
