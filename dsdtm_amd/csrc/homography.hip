// homography.hip — RANSAC homographies for n independent problems in one launch (libdsdtm_amd_homography.so, gfx950).
//
// What one problem is: include/dsdtm_amd_homography.h, "THE DEFINITION" (the shape of cv::findHomography(A, B, CV_RANSAC) at its default
// arguments; which samples are drawn, how ties fall, when the loop stops and how the refit iterates are this project's definition).
// The yardsticks are dsdtm_amd/homography_restatement.py and tests/homography_restatement.c; this file computes the same bits.
//
// One workgroup of 256 threads per problem (blockIdx.x). The points are read once, coalesced, into LDS as doubles (32 bytes per
// correspondence). In a round LANE = HYPOTHESIS: the lane draws its sample (a counter-based integer hash, no shared state), solves the
// four-point system in closed form through the projective basis (branch-free, fixed order, H in nine registers) and walks all m
// points — every lane reads the same LDS address, a broadcast, conflict-free — counting its own inliers. Then one integer atomicMax
// on an LDS word over (count + 1) << 9 | (256 - lane) finds the best count and, among equals, the lowest lane; the winning lane
// parks its H in LDS when it beats the rounds before (strictly: the lowest hypothesis index wins across rounds too) and evaluates the
// stop rule. After the last round the lanes stride over the points for the mask, and the refit runs: per evaluation 30 sums over the
// inliers, each a thread's items in index order, then an LDS tree of fixed shape (no FP64 atomics), and the 8x8 Cholesky on lane 0 with
// the matrix in registers (every loop fully unrolled).
//
// Arithmetic: + - * / sqrt in IEEE double, no contraction (the pragma below), no libm call.
#include "homography.h"

#pragma clang fp contract(off)

namespace dsdtm {

namespace {

constexpr int MAX_POINTS = DSDTM_HOMOGRAPHY_MAX_POINTS;
constexpr int THREADS = HOMOGRAPHY_ROUND;
constexpr int MAX_DRAWS = 16;
constexpr int REFIT_ITERATIONS = 10;
constexpr int RED_BATCH = 6;                               // sums that go through the LDS tree together
constexpr int GN_SUMS = 30;

struct Corr { double ax, ay, bx, by; };

__device__ __forceinline__ bool finite_(double v) { return (v - v) == 0.0; }

__device__ __forceinline__ uint32_t hash3(uint32_t seed, uint32_t k, uint32_t c) {
    uint32_t x = seed + k * 0x9E3779B9u + c * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// the projective basis of four points: columns lambda_i * (x_i, y_i, 1), i = 1..3, with [p1 p2 p3] lambda = p4
__device__ __forceinline__ bool basis(double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3, double (&M)[9]) {
    const double a00 = y1 - y2, a01 = x2 - x1, a02 = x1 * y2 - x2 * y1;
    const double a10 = y2 - y0, a11 = x0 - x2, a12 = x2 * y0 - x0 * y2;
    const double a20 = y0 - y1, a21 = x1 - x0, a22 = x0 * y1 - x1 * y0;
    const double det = (a02 + a12) + a22;
    const double l0 = ((a00 * x3 + a01 * y3) + a02) / det;
    const double l1 = ((a10 * x3 + a11 * y3) + a12) / det;
    const double l2 = ((a20 * x3 + a21 * y3) + a22) / det;
    M[0] = l0 * x0; M[1] = l1 * x1; M[2] = l2 * x2;
    M[3] = l0 * y0; M[4] = l1 * y1; M[5] = l2 * y2;
    M[6] = l0; M[7] = l1; M[8] = l2;
    return det != 0.0 && finite_(det) && l0 != 0.0 && finite_(l0) && l1 != 0.0 && finite_(l1) && l2 != 0.0 && finite_(l2);
}

__device__ __forceinline__ void adj3(const double (&m)[9], double (&a)[9]) {
    a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
    a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
    a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
}

__device__ __forceinline__ void mul3(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// H / H[8]; false when H[8] is zero or an entry is not finite
__device__ __forceinline__ bool normalise(double (&H)[9]) {
    const double s = H[8];
    bool ok = s != 0.0 && finite_(s);
#pragma unroll
    for (int i = 0; i < 9; ++i) { H[i] = H[i] / s; ok = ok && finite_(H[i]); }
    return ok;
}

__device__ __forceinline__ int inlier(const double (&H)[9], const Corr& p, double thr2) {
    const double w = (H[6] * p.ax + H[7] * p.ay) + H[8];
    const double px = ((H[0] * p.ax + H[1] * p.ay) + H[2]) / w, py = ((H[3] * p.ax + H[4] * p.ay) + H[5]) / w;
    const double dx = p.bx - px, dy = p.by - py;
    return (dx * dx + dy * dy) <= thr2 ? 1 : 0;
}

// NQ per-thread partials -> NQ sums at out[0..NQ): the tree 128, 64, ... 1 over the threads, in that shape whatever the problem
template <int NQ>
__device__ __forceinline__ void tree_sums(const double* v, double (*red)[THREADS], double* out, int tid) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q][tid] = v[q];
    __syncthreads();
#pragma unroll
    for (int stride = THREADS / 2; stride >= 1; stride /= 2) {
        if (tid < stride) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q][tid] = red[q][tid] + red[q][tid + stride];
        }
        __syncthreads();
    }
    if (tid < NQ) out[tid] = red[tid][0];
    __syncthreads();
}

// the 30 sums of one Gauss-Newton evaluation at h (LDS, h[8] = 1), points normalised by c = (cxa, cya, cxb, cyb, sa, sb), into out[0..30)
__device__ __forceinline__ void gn_sums(const double* h, const double* c, const Corr* pt, const uint8_t* in, int m,
                                        double (*red)[THREADS], double* out, int tid) {
    double acc[GN_SUMS];
#pragma unroll
    for (int q = 0; q < GN_SUMS; ++q) acc[q] = 0.0;
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
    const double cxa = c[0], cya = c[1], cxb = c[2], cyb = c[3], sa = c[4], sb = c[5];
    for (int i = tid; i < m; i += THREADS) {
        if (!in[i]) continue;
        const Corr p = pt[i];
        const double x = (p.ax - cxa) * sa, y = (p.ay - cya) * sa, bu = (p.bx - cxb) * sb, bv = (p.by - cyb) * sb;
        const double w = (h6 * x + h7 * y) + 1.0;
        const double u = ((h0 * x + h1 * y) + h2) / w, v = ((h3 * x + h4 * y) + h5) / w;
        const double ru = u - bu, rv = v - bv;
        const double iw = 1.0 / w, a = x * iw, b = y * iw, cc = iw;
        const double p6 = u * a, p7 = u * b, q6 = v * a, q7 = v * b;
        const double t[GN_SUMS] = {a * a, a * b, a * cc, b * b, b * cc, cc * cc,
                                   a * p6, a * p7, b * p6, b * p7, cc * p6, cc * p7,
                                   a * q6, a * q7, b * q6, b * q7, cc * q6, cc * q7,
                                   p6 * p6 + q6 * q6, p6 * p7 + q6 * q7, p7 * p7 + q7 * q7,
                                   a * ru, b * ru, cc * ru, a * rv, b * rv, cc * rv,
                                   p6 * ru + q6 * rv, p7 * ru + q7 * rv, ru * ru + rv * rv};
#pragma unroll
        for (int q = 0; q < GN_SUMS; ++q) acc[q] = acc[q] + t[q];
    }
#pragma unroll
    for (int b = 0; b < GN_SUMS / RED_BATCH; ++b) tree_sums<RED_BATCH>(&acc[RED_BATCH * b], red, out + RED_BATCH * b, tid);
}

// J^T J x = J^T r by Cholesky from the 30 sums (one lane; every index is static after unrolling, so A, L, y and x are registers);
// false at a non-positive pivot or a non-finite entry of x
__device__ __forceinline__ bool solve_step(const double* S, double (&x)[8]) {
    double A[8][8], L[8][8], g[8], yv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { A[i][j] = 0.0; L[i][j] = 0.0; }
    A[0][0] = S[0]; A[0][1] = S[1]; A[0][2] = S[2]; A[1][1] = S[3]; A[1][2] = S[4]; A[2][2] = S[5];
    A[3][3] = S[0]; A[3][4] = S[1]; A[3][5] = S[2]; A[4][4] = S[3]; A[4][5] = S[4]; A[5][5] = S[5];
    A[0][6] = -S[6]; A[0][7] = -S[7]; A[1][6] = -S[8]; A[1][7] = -S[9]; A[2][6] = -S[10]; A[2][7] = -S[11];
    A[3][6] = -S[12]; A[3][7] = -S[13]; A[4][6] = -S[14]; A[4][7] = -S[15]; A[5][6] = -S[16]; A[5][7] = -S[17];
    A[6][6] = S[18]; A[6][7] = S[19]; A[7][7] = S[20];
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = S[21 + i];
    g[6] = -S[27]; g[7] = -S[28];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        ok = ok && s > 0.0 && finite_(s);
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double t = A[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double s = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * yv[k];
        yv[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = yv[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
        ok = ok && finite_(x[i]);
    }
    return ok;
}

__global__ __launch_bounds__(THREADS) void homography_kernel(const HomographyDev* __restrict__ recs) {
    __shared__ Corr s_pt[MAX_POINTS];                       // 64 KB
    __shared__ double s_red[RED_BATCH][THREADS];            // 12 KB
    __shared__ uint8_t s_in[MAX_POINTS];                    // 2 KB
    __shared__ double s_bestH[9], s_h[9], s_t[9], s_c[6], s_S[GN_SUMS], s_sum[GN_SUMS];
    __shared__ unsigned s_key;
    __shared__ int s_best_count, s_best_k, s_rounds, s_stop, s_go, s_accept, s_iters;

    const HomographyDev r = recs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    // (the host checked both; they bound the LDS arrays and the loops here)
    const int m = min(r.m, MAX_POINTS), rounds_max = min(r.rounds_max, HOMOGRAPHY_MAX_ROUNDS);
    dsdtm_homography_result* __restrict__ out = r.out;
    if (m <= 4) {                                            // the reference's tPointsA.size() > 4
        if (tid == 0) out->found = 0;
        return;
    }
    for (int i = tid; i < m; i += THREADS) {
        const float2 a = ((const float2*)r.a)[i], b = ((const float2*)r.b)[i];
        s_pt[i] = Corr{(double)a.x, (double)a.y, (double)b.x, (double)b.y};
    }
    if (tid == 0) { s_best_count = -1; s_best_k = -1; s_rounds = 0; s_stop = 0; s_key = 0u; }
    __syncthreads();

    const double thr2 = r.thr2;
    for (int round = 0; round < HOMOGRAPHY_MAX_ROUNDS; ++round) {
        if (round >= rounds_max) break;
        const uint32_t k = (uint32_t)(round * THREADS + tid);
        // the sample: a repeated index is redrawn with the next counter; 16 draws at most
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0, got = 0;
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)MAX_DRAWS; ++c) {
            const int i = (int)__umulhi(hash3(r.seed, k, c), (uint32_t)m);
            const bool fresh = got < 4 && (got < 1 || s0 != i) && (got < 2 || s1 != i) && (got < 3 || s2 != i);
            s0 = fresh && got == 0 ? i : s0;
            s1 = fresh && got == 1 ? i : s1;
            s2 = fresh && got == 2 ? i : s2;
            s3 = fresh && got == 3 ? i : s3;
            got += fresh ? 1 : 0;
        }
        double H[9];
        bool valid = got == 4;
        {
            const Corr p0 = s_pt[s0], p1 = s_pt[s1], p2 = s_pt[s2], p3 = s_pt[s3];
            double A[9], B[9], adjA[9];
            const bool okA = basis(p0.ax, p0.ay, p1.ax, p1.ay, p2.ax, p2.ay, p3.ax, p3.ay, A);
            const bool okB = basis(p0.bx, p0.by, p1.bx, p1.by, p2.bx, p2.by, p3.bx, p3.by, B);
            adj3(A, adjA);
            mul3(B, adjA, H);
            const bool okH = normalise(H);
            valid = valid && okA && okB && okH;
        }
        int count = 0;
        for (int i = 0; i < m; ++i) count += inlier(H, s_pt[i], thr2);
        count = valid ? count : -1;
        const unsigned key = ((unsigned)(count + 1) << 9) | (unsigned)(THREADS - tid);           // never 0: s_key is 0 between rounds
        atomicMax(&s_key, key);
        __syncthreads();
        if (key == s_key) {                                  // one lane: the largest count, the lowest lane among equals
            int best = s_best_count;
            if (count > best) {
                best = count;
                s_best_count = count;
                s_best_k = (int)k;
#pragma unroll
                for (int j = 0; j < 9; ++j) s_bestH[j] = H[j];
            }
            const int rounds = round + 1, cnt = best < 0 ? 0 : best;
            s_rounds = rounds;
            bool stop = cnt == m;
            const double w = (double)cnt / (double)m, q = 1.0 - (w * w) * (w * w);
            double p = q;
#pragma unroll
            for (int j = 0; j < 8; ++j) p = p * p;
            double t = p;
            for (int j = 1; j < HOMOGRAPHY_MAX_ROUNDS; ++j) t = j < rounds ? t * p : t;
            stop = stop || t <= r.left;
            s_stop = stop ? 1 : 0;
            s_key = 0u;
        }
        __syncthreads();
        if (s_stop) break;
    }

    const int n_in = s_best_count;
    if (n_in < 4) {                                          // no valid hypothesis: nothing but `found` is written
        if (tid == 0) out->found = 0;
        return;
    }
    double bestH[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) bestH[j] = s_bestH[j];
    for (int i = tid; i < m; i += THREADS) {                 // the mask is the RANSAC model's
        const uint8_t f = (uint8_t)inlier(bestH, s_pt[i], thr2);
        s_in[i] = f;
        r.mask[i] = f;
    }
    __syncthreads();

    // ---- the refit: Hartley normalisation, then Gauss-Newton over h[0..8) with h[8] = 1 ----
    {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < m; i += THREADS) {
            if (!s_in[i]) continue;
            const Corr p = s_pt[i];
            acc[0] = acc[0] + p.ax; acc[1] = acc[1] + p.ay; acc[2] = acc[2] + p.bx; acc[3] = acc[3] + p.by;
        }
        tree_sums<4>(acc, s_red, s_sum, tid);
        if (tid < 4) s_c[tid] = s_sum[tid] / (double)n_in;
        __syncthreads();
    }
    {
        double acc[2] = {0.0, 0.0};
        const double cxa = s_c[0], cya = s_c[1], cxb = s_c[2], cyb = s_c[3];
        for (int i = tid; i < m; i += THREADS) {
            if (!s_in[i]) continue;
            const Corr p = s_pt[i];
            const double dx = p.ax - cxa, dy = p.ay - cya, du = p.bx - cxb, dv = p.by - cyb;
            acc[0] = acc[0] + sqrt(dx * dx + dy * dy);
            acc[1] = acc[1] + sqrt(du * du + dv * dv);
        }
        tree_sums<2>(acc, s_red, s_sum, tid);
    }
    if (tid == 0) {
        const double sa = 1.4142135623730951 / (s_sum[0] / (double)n_in), sb = 1.4142135623730951 / (s_sum[1] / (double)n_in);
        s_c[4] = sa; s_c[5] = sb;
        const bool scales_ok = sa > 0.0 && finite_(sa) && sb > 0.0 && finite_(sb);
        const double Tb[9] = {sb, 0.0, -(sb * s_c[2]), 0.0, sb, -(sb * s_c[3]), 0.0, 0.0, 1.0};
        const double Tai[9] = {1.0 / sa, 0.0, s_c[0], 0.0, 1.0 / sa, s_c[1], 0.0, 0.0, 1.0};
        double t[9], h[9];
        mul3(bestH, Tai, t);
        mul3(Tb, t, h);
        const bool ok = normalise(h);
#pragma unroll
        for (int j = 0; j < 9; ++j) s_h[j] = h[j];
        s_go = scales_ok && ok ? 1 : 0;
        s_iters = 0;
    }
    __syncthreads();
    double cost_before = 0.0, cost_after = 0.0;              // (lane 0's)
    if (s_go) {
        gn_sums(s_h, s_c, s_pt, s_in, m, s_red, s_S, tid);
        const double sb2 = s_c[5] * s_c[5];
        cost_before = cost_after = s_S[GN_SUMS - 1] / sb2;
        for (int it = 0; it < REFIT_ITERATIONS; ++it) {
            if (tid == 0) {
                double x[8];
                const bool ok = solve_step(s_S, x);
#pragma unroll
                for (int j = 0; j < 8; ++j) s_t[j] = s_h[j] - x[j];
                s_t[8] = 1.0;
                s_go = ok ? 1 : 0;
            }
            __syncthreads();
            if (!s_go) break;
            gn_sums(s_t, s_c, s_pt, s_in, m, s_red, s_sum, tid);
            if (tid == 0) {
                if (s_sum[GN_SUMS - 1] < s_S[GN_SUMS - 1]) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) s_h[j] = s_t[j];
                    for (int j = 0; j < GN_SUMS; ++j) s_S[j] = s_sum[j];
                    s_iters = s_iters + 1;
                    s_accept = 1;
                } else s_accept = 0;
            }
            __syncthreads();
            if (!s_accept) break;                            // (a flag of its own: lane 0 may already be writing the next s_go)
        }
        cost_after = s_S[GN_SUMS - 1] / sb2;
    }
    if (tid == 0) {
        int iters = s_iters;
        double Hn[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) Hn[j] = bestH[j];
        if (iters > 0) {
            const double sa = s_c[4], sb = s_c[5];
            const double Tbi[9] = {1.0 / sb, 0.0, s_c[2], 0.0, 1.0 / sb, s_c[3], 0.0, 0.0, 1.0};
            const double Ta[9] = {sa, 0.0, -(sa * s_c[0]), 0.0, sa, -(sa * s_c[1]), 0.0, 0.0, 1.0};
            double h[9], t[9], d[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) h[j] = s_h[j];
            mul3(h, Ta, t);
            mul3(Tbi, t, d);
            if (normalise(d)) {
#pragma unroll
                for (int j = 0; j < 9; ++j) Hn[j] = d[j];
            } else {
                iters = 0;
                cost_after = cost_before;
            }
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) out->H[j] = Hn[j];
        out->cost_before = cost_before; out->cost_after = cost_after;
        out->found = 1; out->n_inliers = n_in; out->best_hypothesis = s_best_k; out->rounds = s_rounds;
        out->refit_iterations = iters; out->reserved = 0;
    }
}

}  // namespace

hipError_t homography_launch(const HomographyDev* recs, int n, hipStream_t stream) {
    hipLaunchKernelGGL(homography_kernel, dim3((unsigned)n), dim3(THREADS), 0, stream, recs);
    return hipGetLastError();
}

}  // namespace dsdtm
