// superpoint_head.hip — everything behind SuperPoint's two convolution heads: the 65-way softmax and depth-to-space of the score
// head, the three-round non-maximum suppression, the threshold / border / top-k selection of the keypoints and the bilinear
// descriptor sampling with its two normalisations, sparse (per keypoint) and dense (per pixel).  Nothing is read back: the
// count of candidates decides the order of the keypoints on the device.  Definition: include/splatraster.h (splatraster_sp_*)
// and INTEGRATION.md §24.
//
// gfx950 shape.
//  * sp_scores_kernel: one lane per 8 x 8 cell.  The lane holds the cell's 65 logits in registers (loads coalesce over the cells of
//    a row), so the maximum, the sum in ascending channel order and the division never cross lanes; it writes eight 32-byte rows.
//  * sp_nms_kernel: one workgroup per tile of outputs, all three rounds fused.  A result depends on S within 5 r pixels, so the
//    panel is the tile plus a 5 r halo: S and one float scratch plane for the separable maxima (row pass into the scratch, column
//    pass on the fly) and three byte planes (mask, suppression, the mask's row pass).  Two instantiations: 64 x 64 tiles up to r = 4
//    (104 x 104 panel: 2 x 43 KB + 3 x 11 KB = 119 KB of the CU's 160 KB, one workgroup of 1024 lanes per CU) and 32 x 32 tiles up
//    to r = 8 (112 x 112 panel, 138 KB).  Pixels outside the image are -inf for the float maxima and 0 for the masks: the clipped
//    window of max_pool2d.  What a pass computes within r of a panel edge that is not an image edge is wrong and never reaches the
//    tile (each of the five passes eats r of the halo).
//  * selection: sp_compact_kernel (a counting and a writing instantiation) and sp_offsets_kernel leave every image's
//    candidates as (score bits, pixel) in row-major order (2048 pixels per workgroup, eight consecutive pixels per lane, a workgroup scan; one workgroup per image
//    scans the chunk counts and writes n and min(n, K)).  sp_pick_kernel, one workgroup per image: n <= K copies the list out;
//    otherwise four 8-bit digit passes over the list (scan.h's radix_select_block: LDS histogram, one wave picks the digit from the
//    top) find the K-th largest score's bits T and its rank among the scores equal to T, and a second walk keeps, in row-major
//    order, every score above T and the equal ones up to that rank.  sp_rank_kernel then gives each of the K survivors its place by counting:
//    the survivors with a larger score plus the equal ones in front of it.  That is the stable descending sort, K^2 comparisons
//    out of LDS (16 M at K = 4096), one launch for the whole batch, and it needs no segmented sort.  Candidates are positive
//    floats, so their bits order as unsigned integers.
//  * sp_normalize_kernel: coarse [B,256,Hc,Wc] -> unit vectors in channel-last order [B,Hc Wc,256] (32 cells per workgroup, the
//    transposition through LDS, the sum of squares in double), so that a neighbour is one contiguous 1 KB read.
//  * sp_sample_kernel / sp_dense_kernel: one wave per point, four channels per lane (sp_describe, the same device function for
//    both, hence bit-identical results).  The sparse kernel transposes 16 keypoints through LDS for the [B,256,K] layout; the dense
//    kernel gives a wave 16 consecutive pixels, keeps the four neighbours in registers while the cell does not change and writes
//    1 KB per pixel with non-temporal stores.
// Compiled without FP contraction: floor(ix) of a keypoint must agree with the CPU restatement (tests/superpoint_reference.py).
#include "common.h"
#include "scan.h"

#include <math.h>

namespace sr {

constexpr int SP_CELL = 8, SP_SEMI = 65, SP_DESC = 256;
constexpr int SP_MAX_RADIUS = 8, SP_MAX_KEYPOINTS = 65535;
constexpr int64_t SP_MAX_PIXELS = (int64_t)1 << 31;
constexpr int SP_TILE = 64, SP_TILE_RMAX = 4;          // the tile splatraster_sp_nms_tile reports: radii 0..4
constexpr int SP_TILE_WIDE_R = 32;                     // radii 5..8: tiles that divide it
constexpr int SP_NMS_THREADS = 1024;
constexpr int SP_SEL_THREADS = 256, SP_SEL_ITEMS = 8, SP_SEL_CHUNK = SP_SEL_THREADS * SP_SEL_ITEMS;
constexpr int SP_PICK_THREADS = 1024;
constexpr int SP_RANK_THREADS = 256, SP_RANK_TILE = 1024;
constexpr int SP_NORM_CELLS = 32;
constexpr int SP_SAMPLE_POINTS = 16;                   // keypoints per workgroup of sp_sample_kernel
constexpr int SP_DENSE_PIXELS = 64;                    // pixels per workgroup of sp_dense_kernel
constexpr float SP_EPS = 1e-12f;

// ---- scores ----------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
sp_scores_kernel(int64_t total, int Hc, int Wc, const float* __restrict__ semi, float* __restrict__ scores)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int cells = Hc * Wc;
    const int b = (int)(g / cells), cell = (int)(g - (int64_t)b * cells);
    const int i = cell / Wc, j = cell - i * Wc;
    const float* src = semi + (int64_t)b * SP_SEMI * cells + cell;
    float v[SP_SEMI];
#pragma unroll
    for (int c = 0; c < SP_SEMI; ++c) v[c] = src[(int64_t)c * cells];
    float m = v[0];
#pragma unroll
    for (int c = 1; c < SP_SEMI; ++c) m = fmaxf(m, v[c]);
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < SP_SEMI; ++c) {
        v[c] = expf(v[c] - m);
        sum = sum + v[c];
    }
    const int W = SP_CELL * Wc;
    float* dst = scores + (int64_t)b * 64 * cells + (int64_t)(SP_CELL * i) * W + SP_CELL * j;
#pragma unroll
    for (int u = 0; u < SP_CELL; ++u) {
        float4* row = reinterpret_cast<float4*>(dst + (int64_t)u * W);   // 32-byte aligned: W and 8 j are multiples of 8
        row[0] = make_float4(v[8 * u] / sum, v[8 * u + 1] / sum, v[8 * u + 2] / sum, v[8 * u + 3] / sum);
        row[1] = make_float4(v[8 * u + 4] / sum, v[8 * u + 5] / sum, v[8 * u + 6] / sum, v[8 * u + 7] / sum);
    }
}

// ---- NMS -------------------------------------------------------------------------------------------------------------------------

// workgroup t owns tile (t % tx, (t / tx) % ty) of image t / (tx ty)
template <int TS, int RMAX>
__global__ void __launch_bounds__(SP_NMS_THREADS)
sp_nms_kernel(int H, int W, int tx, int ty, int r, const float* __restrict__ S, float* __restrict__ out)
{
    constexpr int PMAX = TS + 10 * RMAX;
    __shared__ float s_s[PMAX * PMAX];
    __shared__ float s_t[PMAX * PMAX];
    __shared__ uint8_t s_m[PMAX * PMAX];
    __shared__ uint8_t s_sp[PMAX * PMAX];
    __shared__ uint8_t s_tb[PMAX * PMAX];
    const int tid = threadIdx.x;
    const int P = TS + 10 * r, n = P * P;   // r <= RMAX: checked by the entry point
    const int tile_x = blockIdx.x % tx, rest = blockIdx.x / tx;
    const int tile_y = rest % ty, b = rest / ty;
    const int x0 = tile_x * TS - 5 * r, y0 = tile_y * TS - 5 * r;
    const float* src = S + (int64_t)b * H * W;
    const float ninf = -INFINITY;

    for (int i = tid; i < n; i += SP_NMS_THREADS) {
        const int py = i / P, px = i - py * P;
        const int y = y0 + py, x = x0 + px;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        s_s[i] = in ? src[(int64_t)y * W + x] : ninf;
        s_m[i] = 0;
    }
    __syncthreads();

    // the value round k suppresses around: S outside the suppressed pixels, 0 on them, -inf outside the image
    auto q_at = [&](int i, bool in) -> float { return in ? (s_sp[i] ? 0.0f : s_s[i]) : ninf; };

    for (int round = 0; round < 3; ++round) {
        if (round > 0) {
            // Supp = pool(M) > 0
            for (int i = tid; i < n; i += SP_NMS_THREADS) {
                const int py = i / P, px = i - py * P;
                const int a = max(px - r, 0), e = min(px + r, P - 1);
                uint8_t m = 0;
                for (int k = a; k <= e; ++k) m |= s_m[py * P + k];
                s_tb[i] = m;
            }
            __syncthreads();
            for (int i = tid; i < n; i += SP_NMS_THREADS) {
                const int py = i / P, px = i - py * P;
                const int a = max(py - r, 0), e = min(py + r, P - 1);
                uint8_t m = 0;
                for (int k = a; k <= e; ++k) m |= s_tb[k * P + px];
                s_sp[i] = m;
            }
            __syncthreads();
        }
        // row maxima of S (round 0) or Q into the scratch plane
        for (int i = tid; i < n; i += SP_NMS_THREADS) {
            const int py = i / P, px = i - py * P;
            const int a = max(px - r, 0), e = min(px + r, P - 1);
            const bool row_in = y0 + py >= 0 && y0 + py < H;
            float m = ninf;
            for (int k = a; k <= e; ++k) {
                const float v = round == 0 ? s_s[py * P + k] : q_at(py * P + k, row_in && x0 + k >= 0 && x0 + k < W);
                m = fmaxf(m, v);
            }
            s_t[i] = m;
        }
        __syncthreads();
        // column maxima, and the round's new maxima
        for (int i = tid; i < n; i += SP_NMS_THREADS) {
            const int py = i / P, px = i - py * P;
            const int a = max(py - r, 0), e = min(py + r, P - 1);
            float m = ninf;
            for (int k = a; k <= e; ++k) m = fmaxf(m, s_t[k * P + px]);
            const int y = y0 + py, x = x0 + px;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            if (round == 0)
                s_m[i] = (in && s_s[i] == m) ? 1 : 0;
            else if (in && !s_sp[i] && q_at(i, true) == m)
                s_m[i] = 1;
        }
        __syncthreads();
    }

    float* dst = out + (int64_t)b * H * W;
    for (int i = tid; i < TS * TS; i += SP_NMS_THREADS) {
        const int ty_ = i / TS, tx_ = i - ty_ * TS;
        const int y = tile_y * TS + ty_, x = tile_x * TS + tx_;
        if (y >= H || x >= W) continue;
        const int p = (ty_ + 5 * r) * P + tx_ + 5 * r;
        dst[(int64_t)y * W + x] = s_m[p] ? s_s[p] : 0.0f;
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------------

struct SpSel {
    int H, W, border, K;
    int64_t pixels;      // H W
    int chunks;          // per image
    float threshold;
};

__device__ __forceinline__ bool sp_candidate(const SpSel& s, int64_t p, float v)
{
    const int row = (int)(p / s.W), col = (int)(p - (int64_t)row * s.W);
    return v > s.threshold && row >= s.border && row < s.H - s.border && col >= s.border && col < s.W - s.border;
}

// workgroup g: chunk g % chunks of image g / chunks; lane t owns pixels [8 t, 8 t + 8) of the chunk
template <bool WRITE>
__global__ void __launch_bounds__(SP_SEL_THREADS)
sp_compact_kernel(SpSel s, const float* __restrict__ nms, uint32_t* __restrict__ counts, uint32_t* __restrict__ ckey,
                  uint32_t* __restrict__ cidx)
{
    __shared__ uint32_t s_wave[SP_SEL_THREADS / 64];
    const int b = blockIdx.x / s.chunks, chunk = blockIdx.x - b * s.chunks;
    const int64_t p0 = (int64_t)chunk * SP_SEL_CHUNK + (int64_t)threadIdx.x * SP_SEL_ITEMS;
    const float* src = nms + (int64_t)b * s.pixels;
    float v[SP_SEL_ITEMS];
    uint32_t flags = 0;
#pragma unroll
    for (int e = 0; e < SP_SEL_ITEMS; ++e) {
        const int64_t p = p0 + e;
        v[e] = p < s.pixels ? src[p] : 0.0f;
        if (p < s.pixels && sp_candidate(s, p, v[e])) flags |= 1u << e;
    }
    uint32_t total;
    const uint32_t at = block_exclusive_scan<SP_SEL_THREADS>((uint32_t)__popc(flags), s_wave, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
        return;
    }
    int64_t pos = (int64_t)b * s.pixels + counts[blockIdx.x] + at;   // counts: the image's exclusive scan by now
#pragma unroll
    for (int e = 0; e < SP_SEL_ITEMS; ++e)
        if (flags & (1u << e)) {
            ckey[pos] = __float_as_uint(v[e]);
            cidx[pos] = (uint32_t)(p0 + e);
            ++pos;
        }
}

// one workgroup per image: the chunk counts become their exclusive scan; n and min(n, K) go out
__global__ void __launch_bounds__(SP_PICK_THREADS)
sp_offsets_kernel(int chunks, int K, uint32_t* __restrict__ counts, int32_t* __restrict__ count, int32_t* __restrict__ candidates)
{
    __shared__ uint32_t s_wave[SP_PICK_THREADS / 64];
    uint32_t* c = counts + (int64_t)blockIdx.x * chunks;
    uint32_t run = 0;
    for (int i0 = 0; i0 < chunks; i0 += SP_PICK_THREADS) {
        const int i = i0 + threadIdx.x;
        const uint32_t v = i < chunks ? c[i] : 0u;
        uint32_t total;
        const uint32_t at = block_exclusive_scan<SP_PICK_THREADS>(v, s_wave, &total);
        if (i < chunks) c[i] = run + at;
        run += total;
        __syncthreads();   // (the next step overwrites the wave sums)
    }
    if (threadIdx.x == 0) {
        candidates[blockIdx.x] = (int32_t)run;   // n <= H W < 2^31
        count[blockIdx.x] = (int32_t)min(run, (uint32_t)K);
    }
}

__device__ __forceinline__ void sp_write_keypoint(int W, uint32_t key, uint32_t idx, float* kp, float* score)
{
    const uint32_t row = idx / (uint32_t)W;
    kp[0] = (float)(idx - row * (uint32_t)W);
    kp[1] = (float)row;
    *score = __uint_as_float(key);
}

// The scan of sp_pick_kernel's walk, its own form (scan.h says why): exclusive scan of one word per lane over the workgroup, wave 0
// scanning the wave sums; s_wave: THREADS / 64 + 1 words.  Ends with a barrier: s_wave is free again.
template <int THREADS>
__device__ __forceinline__ uint32_t sp_walk_scan(uint32_t v, uint32_t* s_wave, uint32_t* total)
{
    constexpr int NW = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const uint32_t w = lane < NW ? s_wave[lane] : 0u;
        const uint32_t wi = wave_inclusive_scan(w);
        if (lane < NW) s_wave[lane] = wi - w;
        if (lane == NW - 1) s_wave[NW] = wi;
    }
    __syncthreads();
    const uint32_t res = s_wave[wave] + incl - v;
    *total = s_wave[NW];
    __syncthreads();
    return res;
}

// one workgroup per image.  n <= K: the row-major list goes out, the rows behind it are zeroed.  n > K: the K survivors go to
// selkey / selidx in row-major order, for sp_rank_kernel.
__global__ void __launch_bounds__(SP_PICK_THREADS)
sp_pick_kernel(SpSel s, const int32_t* __restrict__ candidates, const uint32_t* __restrict__ ckey, const uint32_t* __restrict__ cidx,
               uint32_t* __restrict__ selkey, uint32_t* __restrict__ selidx, float* __restrict__ keypoints, float* __restrict__ scores)
{
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[2];
    __shared__ uint32_t s_wave[SP_PICK_THREADS / 64 + 1];
    const int tid = threadIdx.x, b = blockIdx.x;
    const uint32_t n = (uint32_t)candidates[b], K = (uint32_t)s.K;
    const uint32_t* key = ckey + (int64_t)b * s.pixels;
    const uint32_t* idx = cidx + (int64_t)b * s.pixels;
    float* kp = keypoints + (int64_t)b * K * 2;
    float* sc = scores + (int64_t)b * K;
    if (n <= K) {
        for (uint32_t i = tid; i < K; i += SP_PICK_THREADS) {
            if (i < n) {
                sp_write_keypoint(s.W, key[i], idx[i], kp + 2 * i, sc + i);
            } else {
                kp[2 * i] = 0.0f;
                kp[2 * i + 1] = 0.0f;
                sc[i] = 0.0f;
            }
        }
        return;
    }
    // the K-th largest score (the scores are positive floats: their bits order like they do), and its rank among its equals
    uint32_t rank;
    const uint32_t prefix = radix_select_block<SP_PICK_THREADS, true>(n, [&](uint32_t i) { return key[i]; }, K - 1, s_hist, s_sel, &rank);
    // every score above `prefix`, and the equal ones up to that rank
    uint32_t* okey = selkey + (int64_t)b * K;
    uint32_t* oidx = selidx + (int64_t)b * K;
    uint32_t eq_run = 0, sel_run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += SP_PICK_THREADS) {
        const uint32_t i = i0 + tid;
        const uint32_t u = i < n ? key[i] : 0u;
        const bool eq = i < n && u == prefix;
        uint32_t eq_total, sel_total;
        const uint32_t eq_at = eq_run + sp_walk_scan<SP_PICK_THREADS>(eq ? 1u : 0u, s_wave, &eq_total);
        const bool sel = i < n && (u > prefix || (eq && eq_at <= rank));
        const uint32_t at = sel_run + sp_walk_scan<SP_PICK_THREADS>(sel ? 1u : 0u, s_wave, &sel_total);
        if (sel && at < K) {
            okey[at] = u;
            oidx[at] = idx[i];
        }
        eq_run += eq_total;
        sel_run += sel_total;
    }
}

// images with n > K: survivor i of image b goes to row (survivors with a larger score) + (equal ones in front of it)
__global__ void __launch_bounds__(SP_RANK_THREADS)
sp_rank_kernel(int W, int K, int groups, const int32_t* __restrict__ candidates, const uint32_t* __restrict__ selkey,
               const uint32_t* __restrict__ selidx, float* __restrict__ keypoints, float* __restrict__ scores)
{
    __shared__ __align__(16) uint32_t s_k[SP_RANK_TILE];
    const int b = blockIdx.x / groups, group = blockIdx.x - b * groups;
    if (candidates[b] <= K) return;
    const uint32_t* key = selkey + (int64_t)b * K;
    const int i = group * SP_RANK_THREADS + threadIdx.x;
    const uint32_t mine = i < K ? key[i] : 0u;
    uint32_t rank = 0;
    for (int j0 = 0; j0 < K; j0 += SP_RANK_TILE) {
        __syncthreads();
        for (int j = threadIdx.x; j < SP_RANK_TILE; j += SP_RANK_THREADS) s_k[j] = j0 + j < K ? key[j0 + j] : 0u;   // 0: below every score
        __syncthreads();
        const int before = min(max(i - j0, 0), SP_RANK_TILE);   // entries of the tile in front of i
        for (int j = 0; j < SP_RANK_TILE; j += 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(&s_k[j]);
            rank += (q.x > mine || (q.x == mine && j < before)) ? 1u : 0u;
            rank += (q.y > mine || (q.y == mine && j + 1 < before)) ? 1u : 0u;
            rank += (q.z > mine || (q.z == mine && j + 2 < before)) ? 1u : 0u;
            rank += (q.w > mine || (q.w == mine && j + 3 < before)) ? 1u : 0u;
        }
    }
    if (i < K && rank < (uint32_t)K)
        sp_write_keypoint(W, mine, selidx[(int64_t)b * K + i], keypoints + ((int64_t)b * K + rank) * 2, scores + (int64_t)b * K + rank);
}

// ---- descriptors -----------------------------------------------------------------------------------------------------------------

// workgroup g: cells [32 c, 32 c + 32) of image g / groups; lane t reads channels [32 (t / 32), + 32) of cell t % 32
__global__ void __launch_bounds__(256)
sp_normalize_kernel(int cells, int groups, const float* __restrict__ coarse, float* __restrict__ dhat)
{
    __shared__ float s_d[SP_NORM_CELLS][SP_DESC + 1];
    __shared__ double s_part[SP_DESC / 32][SP_NORM_CELLS];
    __shared__ float s_norm[SP_NORM_CELLS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / groups, cell0 = (blockIdx.x - b * groups) * SP_NORM_CELLS;
    const int c = tid & 31, g = tid >> 5;
    const bool live = cell0 + c < cells;
    const float* src = coarse + (int64_t)b * SP_DESC * cells + cell0 + c;
    double acc = 0.0;
    for (int ch = 32 * g; ch < 32 * g + 32; ++ch) {
        const float v = live ? src[(int64_t)ch * cells] : 0.0f;
        s_d[c][ch] = v;
        acc += (double)v * (double)v;
    }
    s_part[g][c] = acc;
    __syncthreads();
    if (tid < SP_NORM_CELLS) {
        double sum = 0.0;
        for (int k = 0; k < SP_DESC / 32; ++k) sum += s_part[k][tid];
        s_norm[tid] = fmaxf((float)sqrt(sum), SP_EPS);
    }
    __syncthreads();
    float* dst = dhat + ((int64_t)b * cells + cell0) * SP_DESC;
    for (int k = 0; k < SP_NORM_CELLS && cell0 + k < cells; ++k) dst[(int64_t)k * SP_DESC + tid] = s_d[k][tid] / s_norm[k];
}

// The four bilinear taps of pixel position (x, y): the north-west cell (clamped to [-2, Wc] x [-2, Hc]: a finite position far
// outside the grid has no neighbour inside it and gives a zero descriptor) and the weights of nw, ne, sw, se.  The clamp also keeps
// the reads of a non-finite position in bounds, but its weights are NaN and so is its descriptor: outside the contract.
struct SpTaps {
    int cx, cy;
    float w[4];
};

__device__ __forceinline__ SpTaps sp_taps(int Hc, int Wc, float x, float y)
{
    const float gx = ((x - 3.5f) / ((float)(SP_CELL * Wc) - 4.5f)) * 2.0f - 1.0f;
    const float gy = ((y - 3.5f) / ((float)(SP_CELL * Hc) - 4.5f)) * 2.0f - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(Wc - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(Hc - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    SpTaps t;
    t.cx = (int)fminf(fmaxf(fx, -2.0f), (float)Wc);
    t.cy = (int)fminf(fmaxf(fy, -2.0f), (float)Hc);
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix;
    const float wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    t.w[0] = wx0 * wy0;
    t.w[1] = wx1 * wy0;
    t.w[2] = wx0 * wy1;
    t.w[3] = wx1 * wy1;
    return t;
}

// channels [4 lane, 4 lane + 4) of the four cells at and behind (cx, cy).  dhat: the image's unit vectors [Hc Wc][256].  Zero
// padding without a branch: a neighbour outside the grid reads a clamped cell and counts as 0.
__device__ __forceinline__ void sp_neighbours(const float* __restrict__ dhat, int Hc, int Wc, int cx, int cy, int lane, float4* v)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nx = cx + (k & 1), ny = cy + (k >> 1);
        const bool in = nx >= 0 && nx < Wc && ny >= 0 && ny < Hc;
        const int sx = min(max(nx, 0), Wc - 1), sy = min(max(ny, 0), Hc - 1);
        const float4 q = *reinterpret_cast<const float4*>(dhat + ((int64_t)sy * Wc + sx) * SP_DESC + 4 * lane);
        v[k] = make_float4(in ? q.x : 0.0f, in ? q.y : 0.0f, in ? q.z : 0.0f, in ? q.w : 0.0f);
    }
}

// All 64 lanes of a wave: the interpolation of the four neighbours, normalised over the 256 channels
__device__ __forceinline__ float4 sp_blend(const float4* v, const float* w)
{
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc.x = acc.x + v[k].x * w[k];
        acc.y = acc.y + v[k].y * w[k];
        acc.z = acc.z + v[k].z * w[k];
        acc.w = acc.w + v[k].w * w[k];
    }
    double sq = ((double)acc.x * acc.x + (double)acc.y * acc.y) + ((double)acc.z * acc.z + (double)acc.w * acc.w);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
    const float nrm = fmaxf((float)sqrt(sq), SP_EPS);
    return make_float4(acc.x / nrm, acc.y / nrm, acc.z / nrm, acc.w / nrm);
}

// All 64 lanes of a wave: channels [4 lane, 4 lane + 4) of the descriptor at pixel position (x, y)
__device__ __forceinline__ float4 sp_describe(const float* __restrict__ dhat, int Hc, int Wc, float x, float y, int lane)
{
    const SpTaps t = sp_taps(Hc, Wc, x, y);
    float4 v[4];
    sp_neighbours(dhat, Hc, Wc, t.cx, t.cy, lane, v);
    return sp_blend(v, t.w);
}

// workgroup g: keypoints [16 g', 16 g' + 16) of image g / groups -> descriptors [B,256,K]; columns at and beyond count[b] are zero
__global__ void __launch_bounds__(256)
sp_sample_kernel(int Hc, int Wc, int K, int groups, const float* __restrict__ dhat, const float* __restrict__ keypoints,
                 const int32_t* __restrict__ count, float* __restrict__ desc)
{
    __shared__ __align__(16) float s_o[SP_SAMPLE_POINTS][SP_DESC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / groups, k0 = (blockIdx.x - b * groups) * SP_SAMPLE_POINTS;
    const int n = min(max(count[b], 0), K);
    const float* img = dhat + (int64_t)b * Hc * Wc * SP_DESC;
    for (int kk = wave; kk < SP_SAMPLE_POINTS; kk += 4) {
        const int k = k0 + kk;
        float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < n) {
            const float* kp = keypoints + ((int64_t)b * K + k) * 2;
            d = sp_describe(img, Hc, Wc, kp[0], kp[1], lane);
        }
        *reinterpret_cast<float4*>(&s_o[kk][4 * lane]) = d;
    }
    __syncthreads();
    float* dst = desc + ((int64_t)b * SP_DESC + tid) * K + k0;
    for (int kk = 0; kk < SP_SAMPLE_POINTS && k0 + kk < K; ++kk) dst[kk] = s_o[kk][tid];
}

// workgroup g: 64 consecutive pixels of the row range, 16 consecutive ones per wave -> out [B,rows,W,256].  Consecutive pixels of
// a row share their four cells for about eight pixels: the wave keeps the neighbours in registers and reads them again only when
// the north-west cell (or the image) changes.  Same taps, same values, same blend as sp_sample_kernel: the same bits.
__global__ void __launch_bounds__(256)
sp_dense_kernel(int Hc, int Wc, int row0, int64_t per_image /*rows W*/, int64_t total, const float* __restrict__ dhat,
                float* __restrict__ out)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t W = SP_CELL * Wc, per = (uint32_t)per_image, n = (uint32_t)total;   // B H W < 2^31: pixel indices fit 32 bits
    const uint32_t p0 = blockIdx.x * SP_DENSE_PIXELS + wave * (SP_DENSE_PIXELS / 4);
    float4 v[4];
    int have_x = 0, have_y = 0;
    uint32_t have_b = 0xFFFFFFFFu;   // no image yet
    for (int k = 0; k < SP_DENSE_PIXELS / 4; ++k) {
        const uint32_t p = p0 + k;
        if (p >= n) break;
        const uint32_t b = p / per, q = p - b * per;
        const uint32_t row = q / W, col = q - row * W;
        const SpTaps t = sp_taps(Hc, Wc, (float)col, (float)(row0 + (int)row));
        if (b != have_b || t.cx != have_x || t.cy != have_y) {   // wave-uniform
            sp_neighbours(dhat + (int64_t)b * Hc * Wc * SP_DESC, Hc, Wc, t.cx, t.cy, lane, v);
            have_b = b;
            have_x = t.cx;
            have_y = t.cy;
        }
        const float4 d = sp_blend(v, t.w);
        const f4 dv = {d.x, d.y, d.z, d.w};
        __builtin_nontemporal_store(dv, reinterpret_cast<f4*>(out + (int64_t)p * SP_DESC) + lane);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

// workspace: [unit vectors B cells 256 f32 | chunk counts | candidate keys B H W | candidate pixels B H W | survivor keys B K | pixels B K]
struct SpWs {
    float* dhat;
    uint32_t *counts, *ckey, *cidx, *selkey, *selidx;
    size_t dhat_bytes, total;   // dhat_bytes: the first section alone, all that sample / dense_descriptors use
};

static int sp_chunks(int64_t pixels) { return (int)((pixels + SP_SEL_CHUNK - 1) / SP_SEL_CHUNK); }

static SpWs sp_layout(void* base, int64_t B, int64_t H, int64_t W, int64_t K)
{
    const int64_t cells = ((H + SP_CELL - 1) / SP_CELL) * ((W + SP_CELL - 1) / SP_CELL);
    SpWs w;
    Carver c{base};
    w.dhat = c.take<float>((size_t)(B * cells) * SP_DESC);
    w.dhat_bytes = c.o;
    w.counts = c.take<uint32_t>((size_t)(B * sp_chunks(H * W)));
    w.ckey = c.take<uint32_t>((size_t)(B * H * W));
    w.cidx = c.take<uint32_t>((size_t)(B * H * W));
    w.selkey = c.take<uint32_t>((size_t)(B * K));
    w.selidx = c.take<uint32_t>((size_t)(B * K));
    w.total = c.o;
    return w;
}

// B images of H x W pixels: SPLATRASTER_OK, or what is wrong with the shape
static int sp_check_pixels(int64_t B, int64_t H, int64_t W)
{
    if (B < 1 || H < 1 || W < 1) return SPLATRASTER_ERR_BAD_ARG;
    if (H >= SP_MAX_PIXELS || W >= SP_MAX_PIXELS || H * W >= SP_MAX_PIXELS || B * H * W >= SP_MAX_PIXELS) return SPLATRASTER_ERR_UNSUPPORTED;
    return SPLATRASTER_OK;
}

static int sp_check_cells(int32_t B, int32_t Hc, int32_t Wc)
{
    if (B < 1 || Hc < 1 || Wc < 1) return SPLATRASTER_ERR_BAD_ARG;
    return sp_check_pixels(B, (int64_t)Hc * SP_CELL, (int64_t)Wc * SP_CELL);
}

static int launch_sp_normalize(int32_t B, int32_t Hc, int32_t Wc, const float* coarse, float* dhat, hipStream_t stream)
{
    const int cells = Hc * Wc, groups = (cells + SP_NORM_CELLS - 1) / SP_NORM_CELLS;
    hipLaunchKernelGGL(sp_normalize_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, stream, cells, groups, coarse, dhat);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_sp_nms_tile(int32_t* tile_h, int32_t* tile_w)
{
    if (!tile_h || !tile_w) return SPLATRASTER_ERR_BAD_ARG;
    *tile_h = SP_TILE;
    *tile_w = SP_TILE;
    return SPLATRASTER_OK;
}

int splatraster_sp_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t max_keypoints, size_t* bytes)
{
    if (bytes) *bytes = 0;
    if (!bytes || max_keypoints < 1 || max_keypoints > SP_MAX_KEYPOINTS) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_pixels(B, H, W)) return st;
    *bytes = sp_layout(nullptr, B, H, W, max_keypoints).total;
    return SPLATRASTER_OK;
}

int splatraster_sp_scores(int32_t B, int32_t Hc, int32_t Wc, const float* semi, float* scores, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!semi || !scores) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_cells(B, Hc, Wc)) return st;
    if (misaligned(scores, 16)) return SPLATRASTER_ERR_BAD_ARG;   // float4 stores
    const int64_t total = (int64_t)B * Hc * Wc;
    hipLaunchKernelGGL(sp_scores_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, Hc, Wc, semi, scores);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_sp_nms(int32_t B, int32_t H, int32_t W, const float* scores, int32_t radius, float* out, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!scores || !out || radius < 0 || radius > SP_MAX_RADIUS) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_pixels(B, H, W)) return st;
    if (radius == 0) {
        if (out != scores) SR_HIP_CHECK(hipMemcpyAsync(out, scores, (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return SPLATRASTER_OK;
    }
    if (out == scores) return SPLATRASTER_ERR_BAD_ARG;   // a tile reads its neighbours' pixels
    const int ts = radius <= SP_TILE_RMAX ? SP_TILE : SP_TILE_WIDE_R;
    const int tx = (W + ts - 1) / ts, ty = (H + ts - 1) / ts;
    const int64_t blocks = (int64_t)B * tx * ty;   // < 2^31: B H W is
    if (radius <= SP_TILE_RMAX)
        hipLaunchKernelGGL((sp_nms_kernel<SP_TILE, SP_TILE_RMAX>), dim3((unsigned)blocks), dim3(SP_NMS_THREADS), 0, stream, H, W, tx, ty,
                           radius, scores, out);
    else
        hipLaunchKernelGGL((sp_nms_kernel<SP_TILE_WIDE_R, SP_MAX_RADIUS>), dim3((unsigned)blocks), dim3(SP_NMS_THREADS), 0, stream, H, W, tx,
                           ty, radius, scores, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_sp_select(int32_t B, int32_t H, int32_t W, const float* nms, float threshold, int32_t max_keypoints, int32_t border,
                          float* keypoints, float* scores, int32_t* count, int32_t* candidates, void* workspace, size_t workspace_bytes,
                          void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!nms || !keypoints || !scores || !count || !candidates || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (max_keypoints < 1 || max_keypoints > SP_MAX_KEYPOINTS || border < 0 || !(threshold >= 0.0f)) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_pixels(B, H, W)) return st;
    const SpWs w = sp_layout(workspace, B, H, W, max_keypoints);
    if (workspace_bytes < w.total || misaligned(workspace, 16)) return SPLATRASTER_ERR_BAD_ARG;
    uint32_t *counts = w.counts, *ckey = w.ckey, *cidx = w.cidx, *selkey = w.selkey, *selidx = w.selidx;
    SpSel s;
    s.H = H;
    s.W = W;
    s.border = border;
    s.K = max_keypoints;
    s.pixels = (int64_t)H * W;
    s.chunks = sp_chunks(s.pixels);
    s.threshold = threshold;
    const unsigned blocks = (unsigned)((int64_t)B * s.chunks);
    hipLaunchKernelGGL((sp_compact_kernel<false>), dim3(blocks), dim3(SP_SEL_THREADS), 0, stream, s, nms, counts, ckey, cidx);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_offsets_kernel, dim3(B), dim3(SP_PICK_THREADS), 0, stream, s.chunks, s.K, counts, count, candidates);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL((sp_compact_kernel<true>), dim3(blocks), dim3(SP_SEL_THREADS), 0, stream, s, nms, counts, ckey, cidx);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_pick_kernel, dim3(B), dim3(SP_PICK_THREADS), 0, stream, s, (const int32_t*)candidates, (const uint32_t*)ckey,
                       (const uint32_t*)cidx, selkey, selidx, keypoints, scores);
    SR_LAUNCH_CHECK();
    const int groups = (s.K + SP_RANK_THREADS - 1) / SP_RANK_THREADS;
    hipLaunchKernelGGL(sp_rank_kernel, dim3((unsigned)((int64_t)B * groups)), dim3(SP_RANK_THREADS), 0, stream, W, s.K, groups,
                       (const int32_t*)candidates, (const uint32_t*)selkey, (const uint32_t*)selidx, keypoints, scores);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_sp_sample(int32_t B, int32_t Hc, int32_t Wc, const float* coarse, int32_t K, const float* keypoints, const int32_t* count,
                          float* descriptors, void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!coarse || !keypoints || !count || !descriptors || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (K < 1 || K > SP_MAX_KEYPOINTS) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_cells(B, Hc, Wc)) return st;
    const SpWs w = sp_layout(workspace, B, (int64_t)Hc * SP_CELL, (int64_t)Wc * SP_CELL, K);
    if (workspace_bytes < w.dhat_bytes || misaligned(workspace, 16)) return SPLATRASTER_ERR_BAD_ARG;
    float* dhat = w.dhat;
    if (const int st = launch_sp_normalize(B, Hc, Wc, coarse, dhat, stream)) return st;
    const int groups = (K + SP_SAMPLE_POINTS - 1) / SP_SAMPLE_POINTS;
    hipLaunchKernelGGL(sp_sample_kernel, dim3((unsigned)((int64_t)B * groups)), dim3(256), 0, stream, Hc, Wc, K, groups, (const float*)dhat,
                       keypoints, count, descriptors);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_sp_dense_descriptors(int32_t B, int32_t Hc, int32_t Wc, const float* coarse, int32_t row0, int32_t rows, float* out,
                                     void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!coarse || !out || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (const int st = sp_check_cells(B, Hc, Wc)) return st;
    if (row0 < 0 || rows < 1 || (int64_t)row0 + rows > (int64_t)Hc * SP_CELL) return SPLATRASTER_ERR_BAD_ARG;
    const SpWs w = sp_layout(workspace, B, (int64_t)Hc * SP_CELL, (int64_t)Wc * SP_CELL, 1);
    if (workspace_bytes < w.dhat_bytes || misaligned(workspace, 16) || misaligned(out, 16)) return SPLATRASTER_ERR_BAD_ARG;
    float* dhat = w.dhat;
    if (const int st = launch_sp_normalize(B, Hc, Wc, coarse, dhat, stream)) return st;
    const int64_t per_image = (int64_t)rows * Wc * SP_CELL, total = (int64_t)B * per_image;
    hipLaunchKernelGGL(sp_dense_kernel, dim3((unsigned)((total + SP_DENSE_PIXELS - 1) / SP_DENSE_PIXELS)), dim3(256), 0, stream, Hc, Wc, row0,
                       per_image, total, (const float*)dhat, out);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
