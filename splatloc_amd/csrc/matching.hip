// matching.hip — SplatLoc's per-query 2D-3D matching (test.py:247-378: get_frusm_pts, get_ref_keyponts_3d,
// utils/match_utils.py: hungarian_solve): the exact rectangular assignment solver, the descriptor cost matrix and the
// frustum candidates of a database frame.  Definition: include/splatraster.h (splatraster_lsap*, splatraster_match_*,
// splatraster_frustum_*) and INTEGRATION.md §17.
//
// Solver.  scipy's linear_sum_assignment (Crouse's shortest augmenting path) restated for one workgroup per problem.  The
// sequential argmin over the remaining columns becomes one lexicographic key: (spc, tie, column) with tie = 0xFFFF - it for
// an unassigned column (the largest `it` wins) and 0x10000 | it for an assigned one (the smallest wins).  Every thread owns the
// positions it = t + k * LSAP_THREADS of `remaining`; the swap-remove of a step is done by the owner of the removed position, so
// a step costs one barrier (the wave partials are double-buffered).  Step 0 of row `cur` walks the whole row (remaining is
// reset to nc-1..0): it resets spc, checks the row for NaN / -inf, and reads the costs the workgroup prefetched into registers
// during the previous row.  The column / row state lives in LDS (16-bit indices, 128 KiB at nc = 4096) or, for larger
// problems and under splatraster_debug_set_lsap_lds(0), in a global workspace; both paths run the same code.
//
// The whole file is compiled without FP contraction (build.py NO_CONTRACT): the reduced cost ((minVal + c) - u) - v, the
// f64 projections and distances must round like scipy / numpy.
#include "common.h"

#include <math.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace sr {

constexpr int LSAP_THREADS = 1024;
constexpr int LSAP_WAVES = LSAP_THREADS / WAVE;
constexpr int LSAP_PF = 4;                   // costs of the next row's step 0 prefetched per thread (4096 columns)
constexpr int LSAP_BATCH = 64;               // problems per launch (the table travels as a kernel argument)
constexpr int LSAP_LDS_SMALL = 1024;         // the two LDS variants: nc <= 1024 (32 KiB) and nc <= 4096 (128 KiB)
constexpr int LSAP_LDS_LARGE = LSAP_PF * LSAP_THREADS;
constexpr uint32_t LSAP_NONE = 0xFFFFu;      // "-1" of the 16-bit indices (nc <= 65535)

static int g_lsap_lds = 1;   // splatraster_debug_set_lsap_lds

struct LsapEntry {
    int64_t cost_off;   // first element of the oriented [nr, nc] f64 matrix
    int64_t out_off;    // first output slot (nr of them)
    int64_t ws_off;     // byte offset of the global state (global path)
    int32_t nr, nc;     // oriented: nr <= nc
    int32_t transposed;
    int32_t index;      // problem index (status / steps slot)
};

struct LsapBatch {
    LsapEntry e[LSAP_BATCH];
};

// bytes of the global state of one problem: LsapGCol [nc], LsapGRow [nr]
static size_t lsap_state_bytes(int64_t nr, int64_t nc)
{
    return align_up((size_t)nc * 24 + (size_t)nr * 16, 256);
}

__device__ __forceinline__ bool lsap_less(double av, uint64_t ak, double bv, uint64_t bk)
{
    return av < bv || (av == bv && ak < bk);
}

// global-path state: one record per column (rem is indexed by position, which has the same range) and one per row, so the
// kernel keeps two base pointers instead of seven
struct LsapGCol {
    double spc, v;
    uint16_t path, r4c, rem, pad;
};
struct LsapGRow {
    double u;
    uint16_t c4r, pad[3];
};

template <int CAP>
struct LsapState {   // CAP > 0: separate LDS arrays
    double *spc_, *v_, *u_;
    uint16_t *path_, *r4c_, *rem_, *c4r_;
    __device__ double& spc(int j) { return spc_[j]; }
    __device__ double& v(int j) { return v_[j]; }
    __device__ double& u(int i) { return u_[i]; }
    __device__ uint16_t& path(int j) { return path_[j]; }
    __device__ uint16_t& r4c(int j) { return r4c_[j]; }
    __device__ uint16_t& rem(int p) { return rem_[p]; }
    __device__ uint16_t& c4r(int i) { return c4r_[i]; }
};

template <>
struct LsapState<0> {
    LsapGCol* col;
    LsapGRow* row;
    __device__ double& spc(int j) { return col[j].spc; }
    __device__ double& v(int j) { return col[j].v; }
    __device__ double& u(int i) { return row[i].u; }
    __device__ uint16_t& path(int j) { return col[j].path; }
    __device__ uint16_t& r4c(int j) { return col[j].r4c; }
    __device__ uint16_t& rem(int p) { return col[p].rem; }
    __device__ uint16_t& c4r(int i) { return row[i].c4r; }
};

// CAP > 0: state in LDS for nc <= CAP; CAP == 0: state in the global workspace
template <int CAP>
__global__ void __launch_bounds__(LSAP_THREADS)
lsap_kernel(LsapBatch batch, const double* __restrict__ costs, int maximize, int64_t* __restrict__ rows,
            int64_t* __restrict__ cols, int32_t* __restrict__ status, int32_t* __restrict__ steps, char* __restrict__ ws)
{
    constexpr int SCAP = CAP > 0 ? CAP : 1;
    __shared__ double s_spc[SCAP], s_v[SCAP], s_u[SCAP];
    __shared__ uint16_t s_path[SCAP], s_r4c[SCAP], s_rem[SCAP], s_c4r[SCAP];
    __shared__ double s_pv[2][LSAP_WAVES];
    __shared__ uint64_t s_pk[2][LSAP_WAVES];
    __shared__ uint32_t s_cnt[LSAP_WAVES];

    const LsapEntry E = batch.e[blockIdx.x];
    const int nr = E.nr, nc = E.nc;
    const int t = threadIdx.x, wave = t / WAVE, lane = t % WAVE;
    const double* __restrict__ cost = costs + E.cost_off;

    LsapState<CAP> S;
    if constexpr (CAP > 0) {
        S.spc_ = s_spc; S.v_ = s_v; S.u_ = s_u;
        S.path_ = s_path; S.r4c_ = s_r4c; S.rem_ = s_rem; S.c4r_ = s_c4r;
    } else {
        S.col = reinterpret_cast<LsapGCol*>(ws + E.ws_off);
        S.row = reinterpret_cast<LsapGRow*>(S.col + nc);
    }
    const double INF = __builtin_inf();
    const double sgn = maximize ? -1.0 : 1.0;

    for (int j = t; j < nc; j += LSAP_THREADS) { S.v(j) = 0.0; S.r4c(j) = (uint16_t)LSAP_NONE; }
    for (int i = t; i < nr; i += LSAP_THREADS) { S.u(i) = 0.0; S.c4r(i) = (uint16_t)LSAP_NONE; }
    double pf[LSAP_PF];
#pragma unroll
    for (int k = 0; k < LSAP_PF; ++k) {
        const int it = t + k * LSAP_THREADS;
        pf[k] = it < nc ? cost[nc - 1 - it] : 0.0;
    }
    __syncthreads();

    int st = SPLATRASTER_LSAP_OK;
    int32_t nsteps = 0;
    int parity = 0;
    int cur = 0;
    for (; cur < nr; ++cur) {
        int i = cur;
        double ui = S.u(cur);
        double minVal = 0.0;
        int num = nc;
        uint32_t sink = LSAP_NONE;
        bool first = true;
        while (true) {
            double bv = INF;
            uint64_t bk = ~0ull >> 1;   // bit 63 carries the wave's invalid-entry flag
            bool bad = false;
            const double* __restrict__ row = cost + (int64_t)i * nc;
            int k = 0;
            for (int it = t; it < num; it += LSAP_THREADS, ++k) {
                uint32_t j;
                double c;
                if (first) {
                    j = (uint32_t)(nc - 1 - it);
                    S.rem(it) = (uint16_t)j;
                    if (k < LSAP_PF) {
                        c = pf[0];
#pragma unroll
                        for (int q = 1; q < LSAP_PF; ++q)
                            if (q == k) c = pf[q];
                    } else {
                        c = row[j];
                    }
                } else {
                    j = S.rem(it);
                    c = row[j];
                }
                c = c * sgn;
                if (first) bad |= (c != c) || (c == -INF);
                const double r = ((minVal + c) - ui) - S.v(j);
                double s = first ? INF : S.spc(j);
                if (r < s) {
                    S.path(j) = (uint16_t)i;
                    s = r;
                }
                S.spc(j) = s;
                const uint64_t tie = S.r4c(j) == LSAP_NONE ? (uint64_t)(0xFFFFu - (uint32_t)it) : (0x10000ull | (uint32_t)it);
                const uint64_t key = (tie << 16) | j;
                if (lsap_less(s, key, bv, bk)) { bv = s; bk = key; }
            }
            if (first) {
                // the next row's step 0 reads the same positions: start its loads now
                const int nxt = cur + 1 < nr ? cur + 1 : cur;
#pragma unroll
                for (int q = 0; q < LSAP_PF; ++q) {
                    const int it = t + q * LSAP_THREADS;
                    if (it < nc) pf[q] = cost[(int64_t)nxt * nc + (nc - 1 - it)];
                }
            }
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, WAVE);
                const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)bk, o, WAVE);
                if (lsap_less(ov, ok, bv, bk)) { bv = ov; bk = ok; }
            }
            const bool wbad = __any(bad);
            if (lane == 0) {
                s_pv[parity][wave] = bv;
                s_pk[parity][wave] = bk | (wbad ? (1ull << 63) : 0ull);
            }
            __syncthreads();
            double lowest = INF;
            uint64_t key = ~0ull >> 1;
            bool anybad = false;
            for (int w = 0; w < LSAP_WAVES; ++w) {
                const double pv = s_pv[parity][w];
                const uint64_t pk = s_pk[parity][w];
                anybad |= (pk >> 63) != 0;
                const uint64_t kk = pk & (~0ull >> 1);
                if (lsap_less(pv, kk, lowest, key)) { lowest = pv; key = kk; }
            }
            parity ^= 1;
            if (anybad) { st = SPLATRASTER_LSAP_INVALID; break; }
            ++nsteps;
            minVal = lowest;
            if (minVal == INF) { st = SPLATRASTER_LSAP_INFEASIBLE; break; }
            const uint32_t j = (uint32_t)(key & 0xFFFFu);
            const uint32_t tie = (uint32_t)(key >> 16);
            const int index = (tie & 0x10000u) ? (int)(tie & 0xFFFFu) : (int)(0xFFFFu - tie);
            if (index % LSAP_THREADS == t) {
                // swap-remove; the removed column is kept behind `num` (the SC set of this row is rem[num..nc))
                S.rem(index) = S.rem(num - 1);
                S.rem(num - 1) = (uint16_t)j;
            }
            --num;
            const uint32_t rj = S.r4c(j);
            if (rj == LSAP_NONE) { sink = j; break; }
            i = (int)rj;
            ui = S.u(i);
            first = false;
        }
        if (st != SPLATRASTER_LSAP_OK) break;
        __syncthreads();   // rem[num..nc) of the owners' swaps
        // dual update: u[cur] += minVal; SC columns j: v[j] -= minVal - spc[j]; their rows (SR \ {cur}) u += minVal - spc[j]
        for (int p = num + t; p < nc; p += LSAP_THREADS) {
            const uint32_t j = S.rem(p);
            const double d = minVal - S.spc(j);
            if (j != sink) S.u(S.r4c(j)) += d;
            S.v(j) -= d;
        }
        if (t == 0) S.u(cur) += minVal;
        __syncthreads();
        if (t == 0) {
            uint32_t j = sink;
            while (true) {
                const uint32_t pi = S.path(j);
                S.r4c(j) = (uint16_t)pi;
                const uint32_t nj = S.c4r(pi);
                S.c4r(pi) = (uint16_t)j;
                j = nj;
                if ((int)pi == cur) break;
            }
        }
        __syncthreads();
    }
    if (st == SPLATRASTER_LSAP_INFEASIBLE) {
        // scipy rejects invalid entries before it solves: the rows not reached yet decide between the two
        bool bad = false;
        for (int64_t e = (int64_t)(cur + 1) * nc + t; e < (int64_t)nr * nc; e += LSAP_THREADS) {
            const double c = cost[e] * sgn;
            bad |= (c != c) || (c == -INF);
        }
        if (__syncthreads_or(bad)) st = SPLATRASTER_LSAP_INVALID;
    }
    if (t == 0) {
        status[E.index] = st;
        steps[E.index] = nsteps;
    }
    if (st != SPLATRASTER_LSAP_OK) return;
    if (!E.transposed) {
        for (int i = t; i < nr; i += LSAP_THREADS) {
            rows[E.out_off + i] = i;
            cols[E.out_off + i] = S.c4r(i);
        }
        return;
    }
    // transposed: the original rows are the assigned columns, in ascending order
    int64_t base = E.out_off;
    for (int c0 = 0; c0 < nc; c0 += LSAP_THREADS) {
        const int j = c0 + t;
        const uint32_t rr = j < nc ? (uint32_t)S.r4c(j) : LSAP_NONE;
        const bool a = rr != LSAP_NONE;
        const uint64_t m = __ballot(a);
        const uint32_t pre = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int w = 0; w < LSAP_WAVES; ++w) {
            const uint32_t cw = s_cnt[w];
            woff += w < wave ? cw : 0u;
            tot += cw;
        }
        if (a) {
            rows[base + woff + pre] = j;
            cols[base + woff + pre] = rr;
        }
        base += tot;
        __syncthreads();
    }
}

// ---- host: solver -------------------------------------------------------------------------------------------------------
static bool lsap_uses_lds(int32_t nc) { return g_lsap_lds != 0 && nc <= LSAP_LDS_LARGE; }

static int lsap_check(int32_t B, const splatraster_lsap_problem* p)
{
    if (B < 0 || (B > 0 && !p)) return SPLATRASTER_ERR_BAD_ARG;
    for (int32_t b = 0; b < B; ++b) {
        if (p[b].nr < 1 || p[b].nc < p[b].nr || p[b].offset < 0) return SPLATRASTER_ERR_BAD_ARG;
        if (p[b].nc > SPLATRASTER_LSAP_MAX_NC || (int64_t)p[b].nr * p[b].nc >= ((int64_t)1 << 31))
            return SPLATRASTER_ERR_OVERFLOW;
    }
    return SPLATRASTER_OK;
}

// ---- descriptor cost ----------------------------------------------------------------------------------------------------
constexpr int MC_TILE = 64;      // output tile edge
constexpr int MC_KC = 16;        // descriptor dimensions staged per round
constexpr int MC_THREADS = 256;  // 16 x 16 threads, 4 x 4 outputs each (rows ty + 16a, columns tx + 16b)

// F.normalize's denominator max(||x||, 1e-12) of column n of d [D, N]
__global__ void __launch_bounds__(256)
match_norm_kernel(int32_t D, int32_t N, const float* __restrict__ d, float* __restrict__ norm)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int k = 0; k < D; ++k) {
        const float x = d[(int64_t)k * N + n];
        s = fmaf(x, x, s);
    }
    norm[n] = fmaxf(sqrtf(s), 1e-12f);
}

// the f32 similarity of (normalised) column a of A [D, NA] and column b of B [D, NB]: one FMA chain over D, in order.
// match_cost_kernel and match_sims_kernel both compute it this way, so a gathered similarity equals the matrix's.
__device__ __forceinline__ float mc_sim_tail(float acc, float thr) { return acc < thr ? 0.f : acc; }

// cost[r, c] = 1 - sim(R_r, C_c) (f32, sim < thr -> 0) widened to f64; R / C are the oriented row / column sets
__global__ void __launch_bounds__(MC_THREADS)
match_cost_kernel(int32_t D, int32_t NR, int32_t NC, const float* __restrict__ R, const float* __restrict__ nR,
                  const float* __restrict__ Cm, const float* __restrict__ nC, float thr, double* __restrict__ cost)
{
    __shared__ float sa[MC_KC][MC_TILE + 1];
    __shared__ float sb[MC_KC][MC_TILE + 1];
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const int r0 = blockIdx.y * MC_TILE, c0 = blockIdx.x * MC_TILE;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < D; k0 += MC_KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < MC_KC * MC_TILE; e += MC_THREADS) {
            const int kk = e / MC_TILE, x = e % MC_TILE;
            const int k = k0 + kk;
            const int r = r0 + x, c = c0 + x;
            sa[kk][x] = (k < D && r < NR) ? R[(int64_t)k * NR + r] / nR[r] : 0.f;
            sb[kk][x] = (k < D && c < NC) ? Cm[(int64_t)k * NC + c] / nC[c] : 0.f;
        }
        __syncthreads();
        const int kn = min(MC_KC, D - k0);
        for (int kk = 0; kk < kn; ++kk) {
            float av[4], bw[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) av[a] = sa[kk][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) bw[b] = sb[kk][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(av[a], bw[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int r = r0 + ty + 16 * a;
        if (r >= NR) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + tx + 16 * b;
            if (c < NC) cost[(int64_t)r * NC + c] = (double)(1.0f - mc_sim_tail(acc[a][b], thr));
        }
    }
}

// sims[k] = the thresholded similarity of pair (i1[k], i2[k]) of d1 [D, N1], d2 [D, N2]; operands in the order of the
// oriented matrix (rows first) so the chain is the one match_cost_kernel ran (the products are commutative anyway)
__global__ void __launch_bounds__(256)
match_sims_kernel(int32_t D, int32_t N1, int32_t N2, const float* __restrict__ d1, const float* __restrict__ d2,
                  const float* __restrict__ norms, float thr, int64_t K, const int64_t* __restrict__ i1,
                  const int64_t* __restrict__ i2, float* __restrict__ sims)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int64_t a = i1[k], b = i2[k];
    const float na = norms[a], nb = norms[N1 + b];
    float acc = 0.f;
    for (int q = 0; q < D; ++q) acc = fmaf(d1[(int64_t)q * N1 + a] / na, d2[(int64_t)q * N2 + b] / nb, acc);
    sims[k] = mc_sim_tail(acc, thr);
}

// ---- frustum candidates -------------------------------------------------------------------------------------------------
constexpr int FR_THREADS = 256;
constexpr double FR_CELL_INV = 8.0;   // grid cell 0.125 m >= the 0.1 m bound: 27 cells hold every neighbour; x * 8 is exact
constexpr double FR_RADIUS = 0.1;

struct FrCam {
    double w2c[12];   // R row-major, then t
    double K[9];
    double c2w[12];
    double fx, fy, cx, cy;
};

__device__ __forceinline__ uint32_t fr_hash(int64_t x, int64_t y, int64_t z, uint32_t mask)
{
    const uint64_t h = ((uint64_t)x * 73856093ull) ^ ((uint64_t)y * 19349663ull) ^ ((uint64_t)z * 83492791ull);
    return (uint32_t)(h ^ (h >> 32)) & mask;
}

__device__ __forceinline__ int64_t fr_cell(double x) { return (int64_t)floor(x * FR_CELL_INV); }

// per point: projection (f64) and the frustum (and marker) test
__global__ void __launch_bounds__(FR_THREADS)
fr_point_kernel(int64_t N, const float* __restrict__ points, const float* __restrict__ marker, float marker_thr, FrCam cam,
                int32_t W, int32_t H, uint32_t* __restrict__ flags, double2* __restrict__ uv)
{
    const int64_t n = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (n >= N) return;
    const double x = points[n * 3], y = points[n * 3 + 1], z = points[n * 3 + 2];
    const double* m = cam.w2c;
    const double px = m[0] * x + m[1] * y + m[2] * z + m[9];
    const double py = m[3] * x + m[4] * y + m[5] * z + m[10];
    const double pz = m[6] * x + m[7] * y + m[8] * z + m[11];
    const double q0 = cam.K[0] * px + cam.K[1] * py + cam.K[2] * pz;
    const double q1 = cam.K[3] * px + cam.K[4] * py + cam.K[5] * pz;
    const double q2 = cam.K[6] * px + cam.K[7] * py + cam.K[8] * pz;
    const double u = q0 / q2, v = q1 / q2;
    bool keep = pz > 0.05 && 0.0 <= u && u < (double)W && 0.0 <= v && v < (double)H;
    if (marker) keep = keep && marker[n] > marker_thr;
    flags[n] = keep ? 1u : 0u;
    uv[n] = make_double2(u, v);
}

// subset mode: the kept points in index order
__global__ void __launch_bounds__(FR_THREADS)
fr_subset_scatter_kernel(int64_t N, const uint32_t* __restrict__ offs, const uint64_t* __restrict__ total,
                         const float* __restrict__ points, const double2* __restrict__ uv, int32_t* __restrict__ out_idx,
                         float* __restrict__ out_xyz, double* __restrict__ out_uv, int64_t* __restrict__ out_count)
{
    const int64_t n = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (n == 0) *out_count = (int64_t)*total;
    if (n >= N) return;
    const uint32_t next = n + 1 < N ? offs[n + 1] : (uint32_t)*total;
    const uint32_t o = offs[n];
    if (next == o) return;
    out_idx[o] = (int32_t)n;
    out_xyz[(int64_t)o * 3] = points[n * 3];
    out_xyz[(int64_t)o * 3 + 1] = points[n * 3 + 1];
    out_xyz[(int64_t)o * 3 + 2] = points[n * 3 + 2];
    out_uv[(int64_t)o * 2] = uv[n].x;
    out_uv[(int64_t)o * 2 + 1] = uv[n].y;
}

// key mode: the kept points into a hashed uniform grid (counting pass)
__global__ void __launch_bounds__(FR_THREADS)
fr_grid_count_kernel(int64_t N, const uint32_t* __restrict__ offs, const uint64_t* __restrict__ total,
                     const float* __restrict__ points, uint32_t mask, int32_t* __restrict__ cand,
                     uint32_t* __restrict__ cand_hash, uint32_t* __restrict__ counts)
{
    const int64_t n = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (n >= N) return;
    const uint32_t next = n + 1 < N ? offs[n + 1] : (uint32_t)*total;
    const uint32_t o = offs[n];
    if (next == o) return;
    const uint32_t h = fr_hash(fr_cell(points[n * 3]), fr_cell(points[n * 3 + 1]), fr_cell(points[n * 3 + 2]), mask);
    cand[o] = (int32_t)n;
    cand_hash[o] = h;
    atomicAdd(&counts[h], 1u);
}

__global__ void __launch_bounds__(FR_THREADS)
fr_grid_fill_kernel(const uint64_t* __restrict__ total, const uint32_t* __restrict__ cand_hash,
                    const uint32_t* __restrict__ starts, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted)
{
    const uint32_t k = blockIdx.x * FR_THREADS + threadIdx.x;
    if (k >= (uint32_t)*total) return;
    const uint32_t h = cand_hash[k];
    sorted[starts[h] + atomicAdd(&cursor[h], 1u)] = k;
}

// per keypoint pixel (mask == 1): back-projection, nearest kept point (ties: the smaller point index), found if < 0.1 m
// (a back-projection that is not finite or reaches 1e15, from a depth hole, is not searched: no cell index is formed from it)
__global__ void __launch_bounds__(FR_THREADS)
fr_query_kernel(int32_t W, int32_t H, const uint8_t* __restrict__ kp_mask, const float* __restrict__ depth, FrCam cam,
                const float* __restrict__ points, const int32_t* __restrict__ cand, const uint32_t* __restrict__ starts,
                const uint32_t* __restrict__ counts, const uint32_t* __restrict__ sorted, uint32_t mask,
                uint32_t* __restrict__ found, int32_t* __restrict__ best)
{
    const int64_t p = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (p >= (int64_t)W * H) return;
    uint32_t f = 0;
    int32_t bi = -1;
    if (kp_mask[p] == 1) {
        const double row = (double)(p / W), col = (double)(p % W);
        const double d = depth[p];
        const double xs = (col - cam.cx) * d / cam.fx;
        const double ys = (row - cam.cy) * d / cam.fy;
        const double zs = d;
        const double* m = cam.c2w;
        const double qx = m[0] * xs + m[1] * ys + m[2] * zs + m[9];
        const double qy = m[3] * xs + m[4] * ys + m[5] * zs + m[10];
        const double qz = m[6] * xs + m[7] * ys + m[8] * zs + m[11];
        double bd = __builtin_inf();
        if (qx == qx && qy == qy && qz == qz && fabs(qx) < 1e15 && fabs(qy) < 1e15 && fabs(qz) < 1e15) {
            const int64_t cx = fr_cell(qx), cy = fr_cell(qy), cz = fr_cell(qz);
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint32_t h = fr_hash(cx + dx, cy + dy, cz + dz, mask);
                        const uint32_t s0 = starts[h], s1 = s0 + counts[h];
                        for (uint32_t s = s0; s < s1; ++s) {
                            const int32_t n = cand[sorted[s]];
                            const double ex = (double)points[(int64_t)n * 3] - qx;
                            const double ey = (double)points[(int64_t)n * 3 + 1] - qy;
                            const double ez = (double)points[(int64_t)n * 3 + 2] - qz;
                            const double dd = sqrt((ex * ex + ey * ey) + ez * ez);
                            if (dd < bd || (dd == bd && n < bi)) { bd = dd; bi = n; }
                        }
                    }
        }
        f = bd < FR_RADIUS ? 1u : 0u;
    }
    found[p] = f;
    best[p] = bi;
}

__global__ void __launch_bounds__(FR_THREADS)
fr_pair_scatter_kernel(int64_t P, const uint32_t* __restrict__ offs, const uint64_t* __restrict__ total,
                       const int32_t* __restrict__ best, const float* __restrict__ points, const double2* __restrict__ uv,
                       int32_t* __restrict__ out_idx, float* __restrict__ out_xyz, double* __restrict__ out_uv,
                       int64_t* __restrict__ out_count)
{
    const int64_t p = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (p == 0) *out_count = (int64_t)*total;
    if (p >= P) return;
    const uint32_t next = p + 1 < P ? offs[p + 1] : (uint32_t)*total;
    const uint32_t o = offs[p];
    if (next == o) return;
    const int64_t n = best[p];
    out_idx[o] = (int32_t)n;
    out_xyz[(int64_t)o * 3] = points[n * 3];
    out_xyz[(int64_t)o * 3 + 1] = points[n * 3 + 1];
    out_xyz[(int64_t)o * 3 + 2] = points[n * 3 + 2];
    out_uv[(int64_t)o * 2] = uv[n].x;
    out_uv[(int64_t)o * 2 + 1] = uv[n].y;
}

struct FrWs {
    uint32_t *flags, *cand_hash, *counts, *starts, *cursor, *sorted, *found;
    int32_t *cand, *best;
    double2* uv;
    uint64_t *total, *total2;
    void* scan_tmp;
    uint32_t buckets;
    size_t bytes;
};

static FrWs fr_layout(void* base, int64_t N, int64_t P)
{
    FrWs w;
    Carver c{base};
    uint32_t nb = 1024;
    while ((int64_t)nb < N && nb < (1u << 22)) nb <<= 1;
    w.buckets = nb;
    const size_t n = (size_t)(N > 0 ? N : 1), p = (size_t)(P > 0 ? P : 1);
    w.flags = c.take<uint32_t>(n);
    w.uv = c.take<double2>(n);
    w.cand = c.take<int32_t>(n);
    w.cand_hash = c.take<uint32_t>(n);
    w.sorted = c.take<uint32_t>(n);
    w.counts = c.take<uint32_t>(nb);
    w.starts = c.take<uint32_t>(nb);
    w.cursor = c.take<uint32_t>(nb);
    w.found = c.take<uint32_t>(p);
    w.best = c.take<int32_t>(p);
    w.total = c.take<uint64_t>(1);
    w.total2 = c.take<uint64_t>(1);
    const int64_t sn = std::max<int64_t>(std::max<int64_t>(N, P), (int64_t)nb);
    w.scan_tmp = c.take<char>(scan_tmp_bytes(sn));
    w.bytes = c.o;
    return w;
}

static inline unsigned fr_blocks(int64_t n) { return (unsigned)((n + FR_THREADS - 1) / FR_THREADS); }

}  // namespace sr

using namespace sr;

extern "C" {

size_t splatraster_lsap_workspace_bytes(int32_t B, const splatraster_lsap_problem* problems)
{
    if (lsap_check(B, problems) != SPLATRASTER_OK) return 0;
    size_t bytes = 0;
    for (int32_t b = 0; b < B; ++b)
        if (!lsap_uses_lds(problems[b].nc)) bytes += lsap_state_bytes(problems[b].nr, problems[b].nc);
    return bytes;
}

int splatraster_debug_set_lsap_lds(int mode)
{
    g_lsap_lds = mode ? 1 : 0;
    return SPLATRASTER_OK;
}

int splatraster_lsap(int32_t B, const splatraster_lsap_problem* problems, const double* costs, int32_t maximize,
                     int64_t* row_ind, int64_t* col_ind, int32_t* status, int32_t* steps, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int chk = lsap_check(B, problems);
    if (chk != SPLATRASTER_OK) return chk;
    if (B == 0) return SPLATRASTER_OK;
    if (!costs || !row_ind || !col_ind || !status || !steps) return SPLATRASTER_ERR_BAD_ARG;
    if (splatraster_lsap_workspace_bytes(B, problems) > 0 && !workspace) return SPLATRASTER_ERR_BAD_ARG;
    // three groups, one kernel variant each, launched in chunks of LSAP_BATCH problems
    std::vector<LsapEntry> groups[3];
    int64_t out = 0, ws = 0;
    for (int32_t b = 0; b < B; ++b) {
        const splatraster_lsap_problem& p = problems[b];
        LsapEntry e;
        e.cost_off = p.offset;
        e.out_off = out;
        e.ws_off = 0;
        e.nr = p.nr;
        e.nc = p.nc;
        e.transposed = p.transposed ? 1 : 0;
        e.index = b;
        out += p.nr;
        int g;
        if (!lsap_uses_lds(p.nc)) {
            g = 2;
            e.ws_off = ws;
            ws += (int64_t)lsap_state_bytes(p.nr, p.nc);
        } else {
            g = p.nc <= LSAP_LDS_SMALL ? 0 : 1;
        }
        groups[g].push_back(e);
    }
    char* wsp = reinterpret_cast<char*>(workspace);
    for (int g = 0; g < 3; ++g) {
        for (size_t c0 = 0; c0 < groups[g].size(); c0 += LSAP_BATCH) {
            const size_t n = std::min((size_t)LSAP_BATCH, groups[g].size() - c0);
            LsapBatch batch;
            memset(&batch, 0, sizeof(batch));
            for (size_t k = 0; k < n; ++k) batch.e[k] = groups[g][c0 + k];
            if (g == 0)
                hipLaunchKernelGGL(lsap_kernel<LSAP_LDS_SMALL>, dim3((unsigned)n), dim3(LSAP_THREADS), 0, stream, batch, costs,
                                   maximize, row_ind, col_ind, status, steps, wsp);
            else if (g == 1)
                hipLaunchKernelGGL(lsap_kernel<LSAP_LDS_LARGE>, dim3((unsigned)n), dim3(LSAP_THREADS), 0, stream, batch, costs,
                                   maximize, row_ind, col_ind, status, steps, wsp);
            else
                hipLaunchKernelGGL(lsap_kernel<0>, dim3((unsigned)n), dim3(LSAP_THREADS), 0, stream, batch, costs, maximize,
                                   row_ind, col_ind, status, steps, wsp);
            SR_LAUNCH_CHECK();
        }
    }
    return SPLATRASTER_OK;
}

int splatraster_match_cost(int32_t D, int32_t N1, int32_t N2, const float* d1, const float* d2, float threshold, float* norms,
                           double* cost, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (D < 1 || N1 < 1 || N2 < 1 || !d1 || !d2 || !norms || !cost) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(match_norm_kernel, dim3((N1 + 255) / 256), dim3(256), 0, stream, D, N1, d1, norms);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_norm_kernel, dim3((N2 + 255) / 256), dim3(256), 0, stream, D, N2, d2, norms + N1);
    SR_LAUNCH_CHECK();
    const bool tr = N2 < N1;   // the solver's orientation: rows = the smaller set
    const int NR = tr ? N2 : N1, NC = tr ? N1 : N2;
    const float* R = tr ? d2 : d1;
    const float* Cm = tr ? d1 : d2;
    const float* nR = tr ? norms + N1 : norms;
    const float* nC = tr ? norms : norms + N1;
    const dim3 grid((unsigned)((NC + MC_TILE - 1) / MC_TILE), (unsigned)((NR + MC_TILE - 1) / MC_TILE));
    hipLaunchKernelGGL(match_cost_kernel, grid, dim3(MC_THREADS), 0, stream, D, NR, NC, R, nR, Cm, nC, threshold, cost);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_match_sims(int32_t D, int32_t N1, int32_t N2, const float* d1, const float* d2, const float* norms,
                           float threshold, int64_t K, const int64_t* i1, const int64_t* i2, float* sims, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (D < 1 || N1 < 1 || N2 < 1 || K < 0 || !d1 || !d2 || !norms) return SPLATRASTER_ERR_BAD_ARG;
    if (K == 0) return SPLATRASTER_OK;
    if (!i1 || !i2 || !sims) return SPLATRASTER_ERR_BAD_ARG;
    hipLaunchKernelGGL(match_sims_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, D, N1, N2, d1, d2, norms,
                       threshold, K, i1, i2, sims);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

size_t splatraster_frustum_workspace_bytes(int64_t N, int32_t width, int32_t height)
{
    return fr_layout(nullptr, N, (int64_t)(width > 0 ? width : 0) * (height > 0 ? height : 0)).bytes;
}

int splatraster_frustum_candidates(int64_t N, const float* points, const float* marker, float marker_threshold, const double* w2c,
                                   const double* K, int32_t width, int32_t height, const uint8_t* kp_mask, const float* depth,
                                   const double* c2w, const double* kp_K, int32_t* out_idx, float* out_xyz, double* out_uv,
                                   int64_t* out_count, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (N < 0 || width < 1 || height < 1 || !w2c || !K || !out_count || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (N > 0 && (!points || !out_idx || !out_xyz || !out_uv)) return SPLATRASTER_ERR_BAD_ARG;
    const bool key = marker != nullptr;
    if (key && (!kp_mask || !depth || !c2w || !kp_K)) return SPLATRASTER_ERR_BAD_ARG;
    const int64_t P = (int64_t)width * height;
    if (N >= ((int64_t)1 << 31) - 1 || P >= ((int64_t)1 << 31) - 1) return SPLATRASTER_ERR_OVERFLOW;
    if (N == 0) {
        SR_HIP_CHECK(hipMemsetAsync(out_count, 0, sizeof(int64_t), stream));
        return SPLATRASTER_OK;
    }
    FrCam cam;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            cam.w2c[r * 3 + c] = w2c[r * 4 + c];
            cam.K[r * 3 + c] = K[r * 3 + c];
            cam.c2w[r * 3 + c] = key ? c2w[r * 4 + c] : 0.0;
        }
        cam.w2c[9 + r] = w2c[r * 4 + 3];
        cam.c2w[9 + r] = key ? c2w[r * 4 + 3] : 0.0;
    }
    cam.fx = key ? kp_K[0] : 1.0;
    cam.fy = key ? kp_K[1] : 1.0;
    cam.cx = key ? kp_K[2] : 0.0;
    cam.cy = key ? kp_K[3] : 0.0;
    const FrWs w = fr_layout(workspace, N, key ? P : 0);
    hipLaunchKernelGGL(fr_point_kernel, dim3(fr_blocks(N)), dim3(FR_THREADS), 0, stream, N, points, marker, marker_threshold,
                       cam, width, height, w.flags, w.uv);
    SR_LAUNCH_CHECK();
    int st = exclusive_scan_u32(N, w.flags, reinterpret_cast<uint32_t*>(w.total), w.scan_tmp, stream, false);
    if (st != SPLATRASTER_OK) return st;
    if (!key) {
        hipLaunchKernelGGL(fr_subset_scatter_kernel, dim3(fr_blocks(N)), dim3(FR_THREADS), 0, stream, N, w.flags, w.total,
                           points, w.uv, out_idx, out_xyz, out_uv, out_count);
        SR_LAUNCH_CHECK();
        return SPLATRASTER_OK;
    }
    const uint32_t mask = w.buckets - 1;
    SR_HIP_CHECK(hipMemsetAsync(w.counts, 0, (size_t)w.buckets * 4, stream));
    SR_HIP_CHECK(hipMemsetAsync(w.cursor, 0, (size_t)w.buckets * 4, stream));
    hipLaunchKernelGGL(fr_grid_count_kernel, dim3(fr_blocks(N)), dim3(FR_THREADS), 0, stream, N, w.flags, w.total, points,
                       mask, w.cand, w.cand_hash, w.counts);
    SR_LAUNCH_CHECK();
    SR_HIP_CHECK(hipMemcpyAsync(w.starts, w.counts, (size_t)w.buckets * 4, hipMemcpyDeviceToDevice, stream));
    st = exclusive_scan_u32(w.buckets, w.starts, nullptr, w.scan_tmp, stream, false);
    if (st != SPLATRASTER_OK) return st;
    hipLaunchKernelGGL(fr_grid_fill_kernel, dim3(fr_blocks(N)), dim3(FR_THREADS), 0, stream, w.total, w.cand_hash, w.starts,
                       w.cursor, w.sorted);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(fr_query_kernel, dim3(fr_blocks(P)), dim3(FR_THREADS), 0, stream, width, height, kp_mask, depth, cam,
                       points, w.cand, w.starts, w.counts, w.sorted, mask, w.found, w.best);
    SR_LAUNCH_CHECK();
    st = exclusive_scan_u32(P, w.found, reinterpret_cast<uint32_t*>(w.total2), w.scan_tmp, stream, false);
    if (st != SPLATRASTER_OK) return st;
    hipLaunchKernelGGL(fr_pair_scatter_kernel, dim3(fr_blocks(P)), dim3(FR_THREADS), 0, stream, P, w.found, w.total2, w.best,
                       points, w.uv, out_idx, out_xyz, out_uv, out_count);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
