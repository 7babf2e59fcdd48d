// pnp.hip — absolute pose of SplatLoc's localisation (test.py:64-84, solve_pose -> pycolmap.absolute_pose_estimation): P3P
// LO-RANSAC and a Cauchy-loss Levenberg-Marquardt refinement for a batch of problems.  Definition: include/splatraster.h
// (splatraster_pnp*) and INTEGRATION.md §18.
//
// One batch of SPLATRASTER_PNP_BATCH trials per round trip:
//   pnp_hyp_kernel    one lane per (problem, trial): sample, P3P, up to 4 models into the workspace
//   pnp_score_kernel  one wave per model: inlier count and residual sum over the problem's correspondences
//   pnp_best_kernel   one block per problem: the batch's best slot (count, sum, slot) by a fixed-order tree
//   pnp_lo_kernel     one block per problem: compare with the running best, local optimisation, new running best
//   pnp_state_kernel  one block: trials done / required per problem and the "all finished" flag the host reads
// then pnp_mask_kernel (inlier mask of the RANSAC model) and pnp_final_kernel (the robust refinement), one block per problem.
// The normal equations of LO and refinement are per-thread partial sums over a strided share of the inliers, combined by a
// wave butterfly and then the four wave partials in order: fixed order, so every result is bit-identical from run to run.
//
// The whole file is compiled without FP contraction (build.py NO_CONTRACT): the residuals and the minimal solver round like
// the f64 restatement of tests/test_host_pnp.py.
#include "common.h"
#include "reduce.h"

#include <math.h>

#include <algorithm>

namespace sr {

constexpr int PNP_BATCH = SPLATRASTER_PNP_BATCH;
constexpr int PNP_SOL = 4;           // models per trial
constexpr int PNP_MODEL = 12;        // R row-major, t
constexpr int PNP_THREADS = 256;     // blocks of the per-problem kernels (4 waves)
constexpr int PNP_WAVES = PNP_THREADS / WAVE;
constexpr int PNP_LO_ROUNDS = 4;
constexpr int PNP_LO_STEPS = 10;
constexpr int PNP_LM_ITERS = 100;
constexpr int PNP_ACC = 28;          // 21 JtJ (upper triangle, row-major), 6 Jtr, cost

struct PnpState {
    double R[9], t[3];
    double sum;          // residual sum of the running best
    int32_t count;       // inliers of the running best, -1: none yet
    int32_t done;
    int32_t trials;
    int32_t required;
    int32_t batch_slot;  // best slot of the current batch, -1: none
    int32_t pad;
};

// ---------------------------------------------------------------------------------------------------------------- sampler
__device__ __forceinline__ uint64_t pnp_mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ void pnp_sample(uint64_t seed, int64_t trial, int32_t n, int32_t* idx)
{
    const uint64_t s = pnp_mix(seed);
    const uint64_t t3 = (uint64_t)trial * 3ull;
    const int32_t i0 = (int32_t)(pnp_mix(s ^ t3) % (uint64_t)n);
    int32_t i1 = (int32_t)(pnp_mix(s ^ (t3 + 1ull)) % (uint64_t)(n - 1));
    if (i1 >= i0) i1 += 1;
    int32_t i2 = (int32_t)(pnp_mix(s ^ (t3 + 2ull)) % (uint64_t)(n - 2));
    const int32_t lo = min(i0, i1), hi = max(i0, i1);
    if (i2 >= lo) i2 += 1;
    if (i2 >= hi) i2 += 1;
    idx[0] = i0;
    idx[1] = i1;
    idx[2] = i2;
}

// ---------------------------------------------------------------------------------------------------------- minimal solver
// largest real root of x^3 + a x^2 + b x + c
__device__ double pnp_cubic_max_root(double a, double b, double c)
{
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = ((2.0 * a * a * a - 9.0 * a * b) + 27.0 * c) / 54.0;
    const double Q3 = Q * Q * Q;
    double x;
    if (R * R < Q3) {
        const double th = acos(R / sqrt(Q3));
        x = -2.0 * sqrt(Q) * cos((th + 2.0 * M_PI) / 3.0) - a / 3.0;
    } else {
        const double A = -copysign(1.0, R) * cbrt(fabs(R) + sqrt(R * R - Q3));
        const double Bv = A != 0.0 ? Q / A : 0.0;
        x = (A + Bv) - a / 3.0;
    }
    for (int k = 0; k < 2; ++k) {
        const double f = ((x + a) * x + b) * x + c;
        const double d = (3.0 * x + 2.0 * a) * x + b;
        if (d != 0.0) x = x - f / d;
    }
    return x;
}

// real roots of A4 x^4 + A3 x^3 + A2 x^2 + A1 x + A0 (Ferrari), Newton-polished; returns their number (<= 4)
__device__ int pnp_quartic_roots(double A4, double A3, double A2, double A1, double A0, double* out)
{
    const double big = fmax(fmax(fabs(A3), fabs(A2)), fmax(fabs(A1), fabs(A0)));
    if (!isfinite(A4) || !isfinite(big) || !(fabs(A4) > 1e-14 * big)) return 0;
    const double b = A3 / A4, c = A2 / A4, d = A1 / A4, e = A0 / A4;
    const double bb = b * b;
    const double p = c - 0.375 * bb;
    const double q = (d - 0.5 * b * c) + 0.125 * bb * b;
    const double r = ((e - 0.25 * b * d) + 0.0625 * bb * c) - 0.01171875 * bb * bb;
    const double m = pnp_cubic_max_root(p, 0.25 * p * p - r, -0.125 * q * q);
    double ys[4];
    int ny = 0;
    if (m > 1e-14 * (1.0 + fabs(p))) {
        const double s = sqrt(2.0 * m);
        const double h = 0.5 * p + m;
        const double g = q / (2.0 * s);
        for (int k = 0; k < 2; ++k) {
            const double sg = k == 0 ? -1.0 : 1.0;
            const double bq = sg * s, cq = h - sg * g;
            const double disc = bq * bq - 4.0 * cq;
            if (disc >= 0.0) {
                const double sd = sqrt(disc);
                ys[ny++] = 0.5 * (-bq - sd);
                ys[ny++] = 0.5 * (-bq + sd);
            }
        }
    } else {
        const double disc = p * p - 4.0 * r;
        if (disc >= 0.0) {
            const double sd = sqrt(disc);
            for (int k = 0; k < 2; ++k) {
                const double z = k == 0 ? 0.5 * (-p - sd) : 0.5 * (-p + sd);
                if (z >= 0.0) {
                    const double rz = sqrt(z);
                    ys[ny++] = -rz;
                    ys[ny++] = rz;
                }
            }
        }
    }
    for (int k = 0; k < ny; ++k) {
        double x = ys[k] - 0.25 * b;
        for (int it = 0; it < 2; ++it) {
            const double f = (((x + b) * x + c) * x + d) * x + e;
            const double df = ((4.0 * x + 3.0 * b) * x + 2.0 * c) * x + d;
            if (df != 0.0) x = x - f / df;
        }
        out[k] = x;
    }
    return ny;
}

// orthonormal frame (e1, e2, e3) of a triangle as the columns of F (row-major); false when degenerate
__device__ bool pnp_frame(const double* p1, const double* p2, const double* p3, double* F)
{
    const double d1[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double d2[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
    const double n[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    const double l1 = sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2]);
    const double l2 = sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2]);
    const double ln = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(ln > 1e-10 * l1 * l2)) return false;
    const double e1[3] = {d1[0] / l1, d1[1] / l1, d1[2] / l1};
    const double e3[3] = {n[0] / ln, n[1] / ln, n[2] / ln};
    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
    for (int k = 0; k < 3; ++k) {
        F[k * 3 + 0] = e1[k];
        F[k * 3 + 1] = e2[k];
        F[k * 3 + 2] = e3[k];
    }
    return true;
}

// Grunert's P3P: bearings j[3][3] (unit), world points P[3][3]; models [4][12]; returns their number
__device__ int pnp_p3p(const double (*j)[3], const double (*P)[3], double* models)
{
    auto sq = [](const double* a, const double* b) {
        const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
        return (d0 * d0 + d1 * d1) + d2 * d2;
    };
    auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    const double a2 = sq(P[1], P[2]), b2 = sq(P[0], P[2]), c2 = sq(P[0], P[1]);
    if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0)) return 0;
    const double ca = dot(j[1], j[2]), cb = dot(j[0], j[2]), cg = dot(j[0], j[1]);
    const double amc = (a2 - c2) / b2, apc = (a2 + c2) / b2, bmc = (b2 - c2) / b2, bma = (b2 - a2) / b2;
    const double A4 = (amc - 1.0) * (amc - 1.0) - 4.0 * c2 / b2 * ca * ca;
    const double A3 = 4.0 * ((amc * (1.0 - amc) * cb - (1.0 - apc) * ca * cg) + 2.0 * c2 / b2 * ca * ca * cb);
    const double A2 = 2.0 * (((((amc * amc - 1.0) + 2.0 * amc * amc * cb * cb) + 2.0 * bmc * ca * ca) - 4.0 * apc * ca * cb * cg) +
                             2.0 * bma * cg * cg);
    const double A1 = 4.0 * ((-amc * (1.0 + amc) * cb + 2.0 * a2 / b2 * cg * cg * cb) - (1.0 - apc) * ca * cg);
    const double A0 = (1.0 + amc) * (1.0 + amc) - 4.0 * a2 / b2 * cg * cg;
    double vs[4];
    const int nv = pnp_quartic_roots(A4, A3, A2, A1, A0, vs);
    double Fw[9];
    if (!pnp_frame(P[0], P[1], P[2], Fw)) return 0;
    int ns = 0;
    for (int k = 0; k < nv; ++k) {
        const double v = vs[k];
        const double den = 2.0 * (cg - v * ca);
        if (!(v > 0.0) || den == 0.0) continue;
        const double u = (((amc - 1.0) * v * v - 2.0 * amc * cb * v) + 1.0 + amc) / den;
        if (!(u > 0.0)) continue;
        double s1 = sqrt(b2 / ((1.0 + v * v) - 2.0 * v * cb));
        double s2 = u * s1, s3 = v * s1;
        for (int it = 0; it < 3; ++it) {   // Newton on the three cosine-law equations
            const double f0 = ((s1 * s1 + s2 * s2) - 2.0 * s1 * s2 * cg) - c2;
            const double f1 = ((s1 * s1 + s3 * s3) - 2.0 * s1 * s3 * cb) - b2;
            const double f2 = ((s2 * s2 + s3 * s3) - 2.0 * s2 * s3 * ca) - a2;
            const double j00 = 2.0 * (s1 - s2 * cg), j01 = 2.0 * (s2 - s1 * cg), j02 = 0.0;
            const double j10 = 2.0 * (s1 - s3 * cb), j11 = 0.0, j12 = 2.0 * (s3 - s1 * cb);
            const double j20 = 0.0, j21 = 2.0 * (s2 - s3 * ca), j22 = 2.0 * (s3 - s2 * ca);
            const double det = (j00 * (j11 * j22 - j12 * j21) - j01 * (j10 * j22 - j12 * j20)) + j02 * (j10 * j21 - j11 * j20);
            if (!(fabs(det) > 0.0)) break;
            const double d0 = (f0 * (j11 * j22 - j12 * j21) - j01 * (f1 * j22 - j12 * f2)) + j02 * (f1 * j21 - j11 * f2);
            const double d1 = (j00 * (f1 * j22 - j12 * f2) - f0 * (j10 * j22 - j12 * j20)) + j02 * (j10 * f2 - f1 * j20);
            const double d2 = (j00 * (j11 * f2 - f1 * j21) - j01 * (j10 * f2 - f1 * j20)) + f0 * (j10 * j21 - j11 * j20);
            s1 = s1 - d0 / det;
            s2 = s2 - d1 / det;
            s3 = s3 - d2 / det;
        }
        const double C[3][3] = {{j[0][0] * s1, j[0][1] * s1, j[0][2] * s1},
                                {j[1][0] * s2, j[1][1] * s2, j[1][2] * s2},
                                {j[2][0] * s3, j[2][1] * s3, j[2][2] * s3}};
        double Fc[9];
        if (!pnp_frame(C[0], C[1], C[2], Fc)) continue;
        double* m = models + ns * PNP_MODEL;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                m[r * 3 + c] = (Fc[r * 3 + 0] * Fw[c * 3 + 0] + Fc[r * 3 + 1] * Fw[c * 3 + 1]) + Fc[r * 3 + 2] * Fw[c * 3 + 2];
        bool ok = true;
        for (int r = 0; r < 3; ++r) {
            const double cs = (C[0][r] + C[1][r]) + C[2][r];
            const double rp = (m[r * 3 + 0] * ((P[0][0] + P[1][0]) + P[2][0]) + m[r * 3 + 1] * ((P[0][1] + P[1][1]) + P[2][1])) +
                              m[r * 3 + 2] * ((P[0][2] + P[1][2]) + P[2][2]);
            m[9 + r] = (cs - rp) / 3.0;
        }
        for (int q = 0; q < PNP_MODEL; ++q) ok = ok && isfinite(m[q]);
        if (ok) ++ns;
    }
    return ns;
}

// ------------------------------------------------------------------------------------------------------------- residuals
struct PnpPoint {
    double u, v, X0, X1, X2;
};

__device__ __forceinline__ PnpPoint pnp_load(const double* p2, const double* p3, int64_t i)
{
    return {p2[2 * i], p2[2 * i + 1], p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
}

// camera point of X under model m (row-major R, t)
__device__ __forceinline__ void pnp_cam(const double* m, const PnpPoint& p, double& x, double& y, double& z)
{
    x = ((m[0] * p.X0 + m[1] * p.X1) + m[2] * p.X2) + m[9];
    y = ((m[3] * p.X0 + m[4] * p.X1) + m[5] * p.X2) + m[10];
    z = ((m[6] * p.X0 + m[7] * p.X1) + m[8] * p.X2) + m[11];
}

// squared pixel residual; false when z <= 0
__device__ __forceinline__ bool pnp_residual(const splatraster_pnp_problem& pr, const double* m, const PnpPoint& p, double& r)
{
    double x, y, z;
    pnp_cam(m, p, x, y, z);
    const double du = p.u - (pr.fx * (x / z) + pr.cx);
    const double dv = p.v - (pr.fy * (y / z) + pr.cy);
    r = du * du + dv * dv;
    return z > 0.0;
}

__device__ __forceinline__ bool pnp_better(int32_t c1, double s1, int32_t k1, int32_t c2, double s2, int32_t k2)
{
    return c1 > c2 || (c1 == c2 && (s1 < s2 || (s1 == s2 && k1 < k2)));
}

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ void pnp_init_kernel(int32_t B, const splatraster_pnp_problem* probs, PnpState* state)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    PnpState s;
    for (int k = 0; k < 9; ++k) s.R[k] = 0.0;
    for (int k = 0; k < 3; ++k) s.t[k] = 0.0;
    s.sum = 0.0;
    s.count = -1;
    s.done = probs[b].n < 4 ? 1 : 0;
    s.trials = 0;
    s.required = 0;
    s.batch_slot = -1;
    s.pad = 0;
    state[b] = s;
}

__global__ void __launch_bounds__(256) pnp_hyp_kernel(int32_t B, const splatraster_pnp_problem* probs, uint64_t seed, int64_t trial0,
                                                      int32_t ntrials, const double* p2, const double* p3,
                                                      const PnpState* state, int32_t* samples, double* models,
                                                      int32_t* nmodels)
{
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)B * ntrials) return;
    const int b = (int)(id / ntrials);
    if (state && state[b].done) return;
    const splatraster_pnp_problem pr = probs[b];
    int32_t idx[3];
    pnp_sample(seed, trial0 + id % ntrials, pr.n, idx);
    if (samples)
        for (int k = 0; k < 3; ++k) samples[id * 3 + k] = idx[k];
    double j[3][3], P[3][3];
    for (int k = 0; k < 3; ++k) {
        const PnpPoint q = pnp_load(p2, p3, pr.offset + idx[k]);
        const double x = (q.u - pr.cx) / pr.fx, y = (q.v - pr.cy) / pr.fy;
        const double l = sqrt((x * x + y * y) + 1.0);
        j[k][0] = x / l;
        j[k][1] = y / l;
        j[k][2] = 1.0 / l;
        P[k][0] = q.X0;
        P[k][1] = q.X1;
        P[k][2] = q.X2;
    }
    nmodels[id] = pnp_p3p(j, P, models + id * (PNP_SOL * PNP_MODEL));
}

// one wave per model; M models per problem; nmodels (per group of PNP_SOL models) NULL: every model is valid
__global__ void __launch_bounds__(256) pnp_score_kernel(int32_t B, const splatraster_pnp_problem* probs, double thr2, int32_t M,
                                                        const double* models, const int32_t* nmodels, const double* p2,
                                                        const double* p3, const PnpState* state, int32_t* count, double* sum)
{
    const int64_t slot = (int64_t)blockIdx.x * PNP_WAVES + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (slot >= (int64_t)B * M) return;
    const int b = (int)(slot / M);
    if (state && state[b].done) return;
    if (nmodels && (int)(slot % PNP_SOL) >= nmodels[slot / PNP_SOL]) {
        if (lane == 0) {
            count[slot] = -1;
            sum[slot] = 0.0;
        }
        return;
    }
    const splatraster_pnp_problem pr = probs[b];
    double m[PNP_MODEL];
    for (int k = 0; k < PNP_MODEL; ++k) m[k] = models[slot * PNP_MODEL + k];
    int c = 0;
    double s = 0.0;
    for (int i = lane; i < pr.n; i += WAVE) {
        double r;
        if (pnp_residual(pr, m, pnp_load(p2, p3, pr.offset + i), r) && r <= thr2) {
            c += 1;
            s += r;
        }
    }
    c = wave_sum(c);
    s = wave_sum(s);
    if (lane == 0) {
        count[slot] = c;
        sum[slot] = s;
    }
}

__global__ void __launch_bounds__(PNP_THREADS) pnp_best_kernel(int32_t M, const int32_t* count, const double* sum,
                                                               PnpState* state)
{
    __shared__ int32_t sc[PNP_THREADS], sk[PNP_THREADS];
    __shared__ double ss[PNP_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (state[b].done) return;
    int32_t bc = -1, bk = -1;
    double bs = 0.0;
    for (int k = t; k < M; k += PNP_THREADS) {
        const int32_t c = count[(int64_t)b * M + k];
        const double s = sum[(int64_t)b * M + k];
        if (c >= 0 && (bk < 0 || pnp_better(c, s, k, bc, bs, bk))) {
            bc = c;
            bs = s;
            bk = k;
        }
    }
    sc[t] = bc;
    ss[t] = bs;
    sk[t] = bk;
    __syncthreads();
    for (int w = PNP_THREADS / 2; w > 0; w >>= 1) {
        if (t < w && sk[t + w] >= 0 && (sk[t] < 0 || pnp_better(sc[t + w], ss[t + w], sk[t + w], sc[t], ss[t], sk[t]))) {
            sc[t] = sc[t + w];
            ss[t] = ss[t + w];
            sk[t] = sk[t + w];
        }
        __syncthreads();
    }
    if (t == 0) state[b].batch_slot = sk[0];
}

// ------------------------------------------------------------------------------------------------ block normal equations
// Sum over the correspondences that are inliers of m0 (z > 0, r <= thr2) of the weighted normal equations of the pixel
// error at m (left so(3) perturbation of R, additive t).  cauchy: weight 1 / (1 + r), cost log(1 + r); else weight 1, cost r.
// acc (LDS): PNP_ACC values, visible to every thread on return.  Fixed order: thread strides, wave butterfly, waves in order.
__device__ void pnp_accumulate(const splatraster_pnp_problem* prp, const double* p2, const double* p3, double thr2,
                               const double* m0, const double* m, bool cauchy, double* red, double* acc)
{
    const splatraster_pnp_problem pr = *prp;
    const int t = threadIdx.x, lane = t % WAVE, w = t / WAVE;
    double a[PNP_ACC];
    for (int k = 0; k < PNP_ACC; ++k) a[k] = 0.0;
    for (int i = t; i < pr.n; i += PNP_THREADS) {
        const PnpPoint q = pnp_load(p2, p3, pr.offset + i);
        double r0;
        if (!pnp_residual(pr, m0, q, r0) || !(r0 <= thr2)) continue;
        double x, y, z;
        pnp_cam(m, q, x, y, z);
        if (!(z > 0.0)) continue;
        const double ax = x - m[9], ay = y - m[10], az = z - m[11];   // R X
        const double iz = 1.0 / z;
        const double eu = (pr.fx * (x * iz) + pr.cx) - q.u;
        const double ev = (pr.fy * (y * iz) + pr.cy) - q.v;
        const double r = eu * eu + ev * ev;
        const double au = pr.fx * iz, cu = -pr.fx * x * iz * iz;
        const double av = pr.fy * iz, cv = -pr.fy * y * iz * iz;
        // d(x, y, z) / d(wx, wy, wz, tx, ty, tz): rows (0, az, -ay, 1, 0, 0), (-az, 0, ax, 0, 1, 0), (ay, -ax, 0, 0, 0, 1)
        const double Ju[6] = {cu * ay, au * az - cu * ax, -au * ay, au, 0.0, cu};
        const double Jv[6] = {-av * az + cv * ay, -cv * ax, av * ax, 0.0, av, cv};
        const double wt = cauchy ? 1.0 / (1.0 + r) : 1.0;
        int k = 0;
        for (int p = 0; p < 6; ++p)
            for (int q2 = p; q2 < 6; ++q2) a[k++] += wt * (Ju[p] * Ju[q2] + Jv[p] * Jv[q2]);
        for (int p = 0; p < 6; ++p) a[21 + p] += wt * (Ju[p] * eu + Jv[p] * ev);
        a[27] += cauchy ? log1p(r) : r;
    }
    for (int k = 0; k < PNP_ACC; ++k) a[k] = wave_sum(a[k]);
    if (lane == 0)
        for (int k = 0; k < PNP_ACC; ++k) red[w * PNP_ACC + k] = a[k];
    __syncthreads();
    if (t < PNP_ACC) {
        double s = red[t];
        for (int v = 1; v < PNP_WAVES; ++v) s += red[v * PNP_ACC + t];
        acc[t] = s;
    }
    __syncthreads();
}

// support (count, sum) of m over all correspondences, valid in every thread
__device__ void pnp_block_score(const splatraster_pnp_problem* prp, const double* p2, const double* p3, double thr2,
                                const double* m, double* red, int32_t& count, double& sum)
{
    const splatraster_pnp_problem pr = *prp;
    const int t = threadIdx.x, lane = t % WAVE, w = t / WAVE;
    int c = 0;
    double s = 0.0;
    for (int i = t; i < pr.n; i += PNP_THREADS) {
        double r;
        if (pnp_residual(pr, m, pnp_load(p2, p3, pr.offset + i), r) && r <= thr2) {
            c += 1;
            s += r;
        }
    }
    c = wave_sum(c);
    s = wave_sum(s);
    if (lane == 0) {
        red[w * 2] = (double)c;
        red[w * 2 + 1] = s;
    }
    __syncthreads();
    double cc = red[0], ss = red[1];
    for (int v = 1; v < PNP_WAVES; ++v) {
        cc += red[v * 2];
        ss += red[v * 2 + 1];
    }
    count = (int32_t)cc;
    sum = ss;
    __syncthreads();
}

// solve (H + lambda diag(H)) d = -g from the 21 + 6 accumulated values; false when not positive definite
__device__ bool pnp_solve6(const double* acc, double lambda, double* d)
{
    double L[6][6];
    int k = 0;
    for (int p = 0; p < 6; ++p)
        for (int q = p; q < 6; ++q) {
            L[p][q] = acc[k];
            L[q][p] = acc[k];
            ++k;
        }
    for (int p = 0; p < 6; ++p) L[p][p] = L[p][p] + lambda * L[p][p];
    for (int p = 0; p < 6; ++p) {
        double s = L[p][p];
        for (int q = 0; q < p; ++q) s -= L[p][q] * L[p][q];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double l = sqrt(s);
        L[p][p] = l;
        for (int r = p + 1; r < 6; ++r) {
            double v = L[r][p];
            for (int q = 0; q < p; ++q) v -= L[r][q] * L[p][q];
            L[r][p] = v / l;
        }
    }
    double y[6];
    for (int p = 0; p < 6; ++p) {
        double v = -acc[21 + p];
        for (int q = 0; q < p; ++q) v -= L[p][q] * y[q];
        y[p] = v / L[p][p];
    }
    for (int p = 5; p >= 0; --p) {
        double v = y[p];
        for (int q = p + 1; q < 6; ++q) v -= L[q][p] * d[q];
        d[p] = v / L[p][p];
    }
    for (int p = 0; p < 6; ++p)
        if (!isfinite(d[p])) return false;
    return true;
}

// out = (exp([w]x) R, t + dt); out may alias m
__device__ void pnp_apply(const double* m, const double* d, double* out)
{
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double A, Bc;
    if (th2 < 1e-16) {
        A = 1.0 - th2 / 6.0;
        Bc = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        double sn, cs;
        sincos(th, &sn, &cs);
        A = sn / th;
        Bc = (1.0 - cs) / th2;
    }
    const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double E[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double kk = (K[r * 3 + 0] * K[0 * 3 + c] + K[r * 3 + 1] * K[1 * 3 + c]) + K[r * 3 + 2] * K[2 * 3 + c];
            E[r * 3 + c] = ((r == c ? 1.0 : 0.0) + A * K[r * 3 + c]) + Bc * kk;
        }
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = (E[r * 3 + 0] * m[0 * 3 + c] + E[r * 3 + 1] * m[1 * 3 + c]) + E[r * 3 + 2] * m[2 * 3 + c];
    for (int k = 0; k < 9; ++k) out[k] = R[k];
    for (int k = 0; k < 3; ++k) out[9 + k] = m[9 + k] + d[3 + k];
}

__device__ __forceinline__ double pnp_norm6(const double* d)
{
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += d[k] * d[k];
    return sqrt(s);
}

// compare the batch's best with the running best; on improvement local optimisation and a new running best
__global__ void __launch_bounds__(PNP_THREADS) pnp_lo_kernel(const splatraster_pnp_problem* probs, double thr2, int32_t M,
                                                             const double* models, const int32_t* count, const double* sum,
                                                             const double* p2, const double* p3, PnpState* state)
{
    __shared__ double red[PNP_WAVES * PNP_ACC];
    __shared__ double acc[PNP_ACC], step[6];
    __shared__ double cur[PNP_MODEL], start[PNP_MODEL];
    __shared__ splatraster_pnp_problem sp;   // read from LDS inside the loops: keeps the SGPR budget
    __shared__ int ctl;
    const int b = blockIdx.x, t = threadIdx.x;
    PnpState* st = state + b;
    if (st->done) return;
    const int32_t slot = st->batch_slot;
    if (slot < 0) return;
    const int64_t g = (int64_t)b * M + slot;
    int32_t bc = count[g];
    double bs = sum[g];
    // the running best comes from an earlier trial, so it wins every exact tie
    if (!(bc > st->count || (bc == st->count && bs < st->sum))) return;
    if (t < PNP_MODEL) cur[t] = models[g * PNP_MODEL + t];
    if (t == 0) sp = probs[b];
    __syncthreads();
    for (int round = 0; round < PNP_LO_ROUNDS; ++round) {
        if (t < PNP_MODEL) start[t] = cur[t];
        __syncthreads();
        double m[PNP_MODEL];
        for (int k = 0; k < PNP_MODEL; ++k) m[k] = cur[k];
        for (int it = 0; it < PNP_LO_STEPS; ++it) {
            pnp_accumulate(&sp, p2, p3, thr2, start, m, false, red, acc);
            if (t == 0) {   // one thread solves, the block applies the broadcast step
                double d[6];
                const bool ok = pnp_solve6(acc, 0.0, d);
                for (int k = 0; k < 6; ++k) step[k] = d[k];
                ctl = !ok ? 1 : (pnp_norm6(d) < 1e-12 ? 2 : 0);
            }
            __syncthreads();
            const int c = ctl;
            if (c == 1) break;
            pnp_apply(m, step, m);
            if (c == 2) break;
        }
        bool fin = true;
        for (int k = 0; k < PNP_MODEL; ++k) fin = fin && isfinite(m[k]);
        if (!fin) break;
        int32_t c;
        double s;
        pnp_block_score(&sp, p2, p3, thr2, m, red, c, s);
        if (!(c > bc || (c == bc && s < bs))) break;
        bc = c;
        bs = s;
        if (t < PNP_MODEL) cur[t] = m[t];
        __syncthreads();
    }
    if (t == 0) {
        for (int k = 0; k < 9; ++k) st->R[k] = cur[k];
        for (int k = 0; k < 3; ++k) st->t[k] = cur[9 + k];
        st->count = bc;
        st->sum = bs;
    }
}

__global__ void __launch_bounds__(PNP_THREADS) pnp_state_kernel(int32_t B, const splatraster_pnp_problem* probs,
                                                                splatraster_pnp_options opt, PnpState* state, int32_t* all_done)
{
    int open = 0;
    for (int b = threadIdx.x; b < B; b += PNP_THREADS) {
        PnpState* st = state + b;
        if (st->done) continue;
        st->trials += PNP_BATCH;
        const int32_t n = probs[b].n;
        const int32_t k = max(st->count, 0);
        int32_t req;
        const double p = (double)k / (double)n;
        if (k == 0 || p < opt.min_inlier_ratio) {
            req = opt.max_num_trials;
        } else {
            const double p3 = p * p * p;
            if (p3 >= 1.0) {
                req = opt.min_num_trials;
            } else {
                const double den = log(1.0 - p3);
                if (!(den < 0.0)) {
                    req = opt.max_num_trials;
                } else {
                    const double r = ceil(log(1.0 - opt.confidence) / den);
                    req = r <= (double)opt.min_num_trials ? opt.min_num_trials
                        : (r >= (double)opt.max_num_trials ? opt.max_num_trials : (int32_t)r);
                }
            }
        }
        st->required = req;
        st->done = st->trials >= req ? 1 : 0;
        open |= st->done ? 0 : 1;
    }
    open = __syncthreads_or(open);
    if (threadIdx.x == 0) *all_done = open ? 0 : 1;
}

// inlier mask, inlier count and trials of the RANSAC model
__global__ void __launch_bounds__(PNP_THREADS) pnp_mask_kernel(const splatraster_pnp_problem* probs, double thr2,
                                                               const double* p2, const double* p3, const PnpState* state,
                                                               int32_t* num_inliers, uint8_t* mask, int32_t* trials)
{
    __shared__ double m0[PNP_MODEL];
    const int b = blockIdx.x, t = threadIdx.x;
    const PnpState* st = state + b;
    const int32_t cnt = st->count;
    if (t < 9) m0[t] = st->R[t];
    else if (t < PNP_MODEL) m0[t] = st->t[t - 9];
    __syncthreads();
    const bool ok = cnt >= 4;
    const splatraster_pnp_problem pr = probs[b];
    for (int i = t; i < pr.n; i += PNP_THREADS) {
        double r;
        mask[pr.offset + i] = (ok && pnp_residual(pr, m0, pnp_load(p2, p3, pr.offset + i), r) && r <= thr2) ? 1 : 0;
    }
    if (t == 0) {
        num_inliers[b] = max(cnt, 0);
        trials[b] = st->trials;
    }
}

// the Cauchy-loss Levenberg-Marquardt refinement on the inliers of the RANSAC model
__global__ void __launch_bounds__(PNP_THREADS) pnp_final_kernel(const splatraster_pnp_problem* probs, double thr2,
                                                                const double* p2, const double* p3, const PnpState* state,
                                                                double* R_out, double* t_out, int32_t* status)
{
    __shared__ double red[PNP_WAVES * PNP_ACC];
    __shared__ double acc[PNP_ACC], nacc[PNP_ACC], step[6];
    __shared__ double m0[PNP_MODEL];
    __shared__ double lam;
    __shared__ splatraster_pnp_problem sp;   // read from LDS inside the loops: keeps the SGPR budget
    __shared__ int ctl;
    const int b = blockIdx.x, t = threadIdx.x;
    const PnpState* st = state + b;
    const bool ok = st->count >= 4;
    if (t < 9) m0[t] = st->R[t];
    else if (t < PNP_MODEL) m0[t] = st->t[t - 9];
    if (t == 0) sp = probs[b];
    __syncthreads();
    if (!ok) {
        if (t < 9) R_out[b * 9 + t] = 0.0;
        if (t < 3) t_out[b * 3 + t] = 0.0;
        if (t == 0) status[b] = SPLATRASTER_PNP_NO_MODEL;
        return;
    }
    double m[PNP_MODEL];
    for (int k = 0; k < PNP_MODEL; ++k) m[k] = m0[k];
    if (t == 0) lam = 1e-4;
    pnp_accumulate(&sp, p2, p3, thr2, m0, m, true, red, acc);
    // thread 0 decides (ctl): 0 try the step, 1 no step (damping raised), 2 stop, 3 accept and stop, 4 accept, 5 reject
    for (int it = 0; it < PNP_LM_ITERS; ++it) {
        if (t == 0) {   // one thread solves, the block applies the broadcast step
            double d[6];
            const bool solved = pnp_solve6(acc, lam, d);
            for (int k = 0; k < 6; ++k) step[k] = d[k];
            int c = !solved ? 1 : (pnp_norm6(d) < 1e-10 ? 2 : 0);
            if (c == 1) {
                lam *= 10.0;
                if (lam > 1e16) c = 2;
            }
            ctl = c;
        }
        __syncthreads();
        const int c = ctl;
        __syncthreads();
        if (c == 2) break;
        if (c == 1) continue;
        double mn[PNP_MODEL];
        pnp_apply(m, step, mn);
        pnp_accumulate(&sp, p2, p3, thr2, m0, mn, true, red, nacc);
        if (t == 0) {
            const double c0 = acc[27], c1 = nacc[27];
            if (c1 < c0) {
                for (int k = 0; k < PNP_ACC; ++k) acc[k] = nacc[k];
                lam = fmax(lam * 0.1, 1e-12);
                ctl = (c0 - c1) / c0 < 1e-10 ? 3 : 4;
            } else {
                lam *= 10.0;
                ctl = lam > 1e16 ? 2 : 5;
            }
        }
        __syncthreads();
        const int a = ctl;
        __syncthreads();
        if (a == 3 || a == 4)
            for (int k = 0; k < PNP_MODEL; ++k) m[k] = mn[k];
        if (a == 2 || a == 3) break;
    }
    bool fin = true;
    for (int k = 0; k < PNP_MODEL; ++k) fin = fin && isfinite(m[k]);
    if (t < 9) R_out[b * 9 + t] = m[t];
    if (t < 3) t_out[b * 3 + t] = m[9 + t];
    if (t == 0) status[b] = fin ? SPLATRASTER_PNP_OK : SPLATRASTER_PNP_NONFINITE;
}

// ------------------------------------------------------------------------------------------------------------------- host
struct PnpLayout {
    splatraster_pnp_problem* probs;
    PnpState* state;
    double* models;
    int32_t *nmod, *count;
    double* sum;
    int32_t* flag;
    size_t total;
};

static PnpLayout pnp_layout(void* base, int32_t B)
{
    PnpLayout L;
    Carver c{base};
    const size_t slots = (size_t)B * PNP_BATCH * PNP_SOL;
    L.probs = c.take<splatraster_pnp_problem>((size_t)B);
    L.state = c.take<PnpState>((size_t)B);
    L.models = c.take<double>(slots * PNP_MODEL);
    L.nmod = c.take<int32_t>((size_t)B * PNP_BATCH);
    L.count = c.take<int32_t>(slots);
    L.sum = c.take<double>(slots);
    L.flag = c.take<int32_t>(1);
    L.total = c.o;
    return L;
}

static int pnp_check(int32_t B, const splatraster_pnp_problem* p, const splatraster_pnp_options* o)
{
    if (B < 0 || B > 65535 || (B > 0 && (!p || !o))) return SPLATRASTER_ERR_BAD_ARG;
    if (B == 0) return SPLATRASTER_OK;
    if (!(o->max_error_px > 0.0) || !(o->confidence > 0.0 && o->confidence < 1.0) || o->min_num_trials < 1 ||
        o->min_num_trials > o->max_num_trials || !(o->min_inlier_ratio >= 0.0))
        return SPLATRASTER_ERR_BAD_ARG;
    for (int32_t b = 0; b < B; ++b) {
        if (p[b].n < 0 || p[b].offset < 0) return SPLATRASTER_ERR_BAD_ARG;
        if (p[b].n > SPLATRASTER_PNP_MAX_N) return SPLATRASTER_ERR_OVERFLOW;
        if (!(p[b].fx != 0.0 && p[b].fy != 0.0)) return SPLATRASTER_ERR_BAD_ARG;
    }
    return SPLATRASTER_OK;
}

static inline unsigned pnp_blocks(int64_t threads, int per) { return (unsigned)((threads + per - 1) / per); }

}  // namespace sr

using namespace sr;

extern "C" {

size_t splatraster_pnp_workspace_bytes(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options)
{
    if (pnp_check(B, problems, options) != SPLATRASTER_OK || B == 0) return 0;
    return pnp_layout(nullptr, B).total;
}

int splatraster_pnp_hypotheses(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options,
                               int64_t trial0, int32_t ntrials, const double* points2d, const double* points3d, int32_t* samples,
                               double* models, int32_t* nmodels, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int st = pnp_check(B, problems, options);
    if (st != SPLATRASTER_OK || B == 0) return st;
    if (ntrials < 1 || ntrials > PNP_BATCH || trial0 < 0 || !points2d || !points3d || !samples || !models || !nmodels ||
        !workspace)
        return SPLATRASTER_ERR_BAD_ARG;
    for (int32_t b = 0; b < B; ++b)
        if (problems[b].n < 4) return SPLATRASTER_ERR_BAD_ARG;
    const PnpLayout L = pnp_layout(workspace, B);
    splatraster_pnp_problem* probs = L.probs;
    SR_HIP_CHECK(hipMemcpyAsync(probs, problems, (size_t)B * sizeof(*problems), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3(pnp_blocks((int64_t)B * ntrials, 256)), dim3(256), 0, stream, B, probs, options->seed,
                       trial0, ntrials, points2d, points3d, (const PnpState*)nullptr, samples, models, nmodels);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_pnp_score(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options, int32_t M,
                          const double* models, const double* points2d, const double* points3d, int32_t* count, double* sum,
                          void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int st = pnp_check(B, problems, options);
    if (st != SPLATRASTER_OK || B == 0) return st;
    if (M < 0 || (int64_t)B * M > (int64_t)PNP_BATCH * PNP_SOL * B) return SPLATRASTER_ERR_BAD_ARG;
    if (M == 0) return SPLATRASTER_OK;
    if (!models || !points2d || !points3d || !count || !sum || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    const PnpLayout L = pnp_layout(workspace, B);
    splatraster_pnp_problem* probs = L.probs;
    SR_HIP_CHECK(hipMemcpyAsync(probs, problems, (size_t)B * sizeof(*problems), hipMemcpyHostToDevice, stream));
    const double thr2 = options->max_error_px * options->max_error_px;
    hipLaunchKernelGGL(pnp_score_kernel, dim3(pnp_blocks((int64_t)B * M, PNP_WAVES)), dim3(PNP_THREADS), 0, stream, B, probs, thr2,
                       M, models, (const int32_t*)nullptr, points2d, points3d, (const PnpState*)nullptr, count, sum);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

int splatraster_pnp(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options,
                    const double* points2d, const double* points3d, double* R_out, double* t_out, int32_t* num_inliers,
                    uint8_t* inlier_mask, int32_t* status, int32_t* trials, void* workspace, void* stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int st = pnp_check(B, problems, options);
    if (st != SPLATRASTER_OK || B == 0) return st;
    int64_t total = 0;
    for (int32_t b = 0; b < B; ++b) total = std::max(total, problems[b].offset + problems[b].n);
    if (!R_out || !t_out || !num_inliers || !status || !trials || !workspace) return SPLATRASTER_ERR_BAD_ARG;
    if (total > 0 && (!points2d || !points3d || !inlier_mask)) return SPLATRASTER_ERR_BAD_ARG;
    const PnpLayout L = pnp_layout(workspace, B);
    splatraster_pnp_problem* probs = L.probs;
    PnpState* state = L.state;
    double *models = L.models, *sum = L.sum;
    int32_t *nmod = L.nmod, *count = L.count, *flag = L.flag;
    const double thr2 = options->max_error_px * options->max_error_px;
    const int32_t M = PNP_BATCH * PNP_SOL;
    SR_HIP_CHECK(hipMemcpyAsync(probs, problems, (size_t)B * sizeof(*problems), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(pnp_init_kernel, dim3(pnp_blocks(B, 256)), dim3(256), 0, stream, B, probs, state);
    SR_LAUNCH_CHECK();
    bool any = false;
    for (int32_t b = 0; b < B; ++b) any = any || problems[b].n >= 4;
    const int64_t max_batches = ((int64_t)options->max_num_trials + PNP_BATCH - 1) / PNP_BATCH;
    for (int64_t batch = 0; any && batch < max_batches; ++batch) {
        hipLaunchKernelGGL(pnp_hyp_kernel, dim3(pnp_blocks((int64_t)B * PNP_BATCH, 256)), dim3(256), 0, stream, B, probs,
                           options->seed, batch * PNP_BATCH, PNP_BATCH, points2d, points3d, (const PnpState*)state,
                           (int32_t*)nullptr, models, nmod);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pnp_score_kernel, dim3(pnp_blocks((int64_t)B * M, PNP_WAVES)), dim3(PNP_THREADS), 0, stream, B, probs,
                           thr2, M, (const double*)models, (const int32_t*)nmod, points2d, points3d, (const PnpState*)state, count,
                           sum);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pnp_best_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, stream, M, (const int32_t*)count,
                           (const double*)sum, state);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pnp_lo_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, stream, (const splatraster_pnp_problem*)probs,
                           thr2, M, (const double*)models, (const int32_t*)count, (const double*)sum, points2d, points3d, state);
        SR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pnp_state_kernel, dim3(1), dim3(PNP_THREADS), 0, stream, B, (const splatraster_pnp_problem*)probs,
                           *options, state, flag);
        SR_LAUNCH_CHECK();
        int32_t all_done = 0;
        SR_HIP_CHECK(hipMemcpyAsync(&all_done, flag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        SR_HIP_CHECK(hipStreamSynchronize(stream));
        if (all_done) break;
    }
    hipLaunchKernelGGL(pnp_mask_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, stream, (const splatraster_pnp_problem*)probs,
                       thr2, points2d, points3d, (const PnpState*)state, num_inliers, inlier_mask, trials);
    SR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pnp_final_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, stream, (const splatraster_pnp_problem*)probs,
                       thr2, points2d, points3d, (const PnpState*)state, R_out, t_out, status);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // extern "C"
