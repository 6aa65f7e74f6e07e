// rarsac.hip — Rarsac_base::RejectFundamental for n independent problems in one launch (libdsdtm_amd_rarsac.so, gfx950).
//
// What one problem is: include/dsdtm_amd_rarsac.h, rules R1-R9. The yardsticks are dsdtm_amd/rarsac_restatement.py, tests/rarsac_restatement.c
// and dsdtm_amd/host/dsdtm_rarsac_host.hpp; this file computes the same bits.
//
// One workgroup of 256 threads per problem (blockIdx.x). The host sorted the correspondences by bin while it checked them (R1), so the
// kernel stages them once in LDS as float4 and a bin is a range start[j] .. start[j + 1]. In a round LANE = HYPOTHESIS: the lane draws
// its eight bins by inverse CDF over the prefix sums in LDS and a correspondence of each (a counter-based integer hash, no shared
// state), solves the 8x9 system in registers — every array index is a compile-time constant: the pivot row and the pivot column are
// picked out by select chains, so nothing goes to scratch — and walks the correspondences in bin order with ONE running inlier
// counter (every lane reads the same LDS address: a broadcast). The per-bin counts of a lane are parked in LDS as 16-bit words
// ([bin][lane]: conflict-free) because R6 passes over the grid twice. Then thread 0 scans the round's 256 scores IN INDEX ORDER for
// the best-so-far and the stop rule (R7-R9), the winning lane parks its F, and after the last round thread j recounts bin j under the
// winning F for the status and the grid. No FP64 atomics, no atomics at all, nothing waits across workgroups.
//
// Arithmetic: + - * / sqrt in IEEE float and double, no contraction (the pragma below), no libm call.
#include "rarsac.h"

#pragma clang fp contract(off)

namespace dsdtm {

namespace {

constexpr int MAX_POINTS = DSDTM_RARSAC_MAX_POINTS;
constexpr int THREADS = RARSAC_ROUND;
constexpr int GRID = RARSAC_GRID;
constexpr int BIN_DRAWS = 64;
constexpr int JACOBI_SWEEPS = 8;
constexpr double DBL_MIN_ = 2.2250738585072014e-308;

__device__ __forceinline__ uint32_t hash3(uint32_t seed, uint32_t k, uint32_t c) {
    uint32_t x = seed + k * 0x9E3779B9u + c * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// R5: whether a correspondence is an inlier of F (float32, as written; a NaN distance does not reject)
__device__ __forceinline__ int inlier(const float (&F)[9], const float4 p, float inv_sigma2) {
    const float th = 3.841f;
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_sigma2;
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_sigma2;
    return (chi1 > th || chi2 > th) ? 0 : 1;
}

__device__ __forceinline__ double grid_p(int b, int a) {
    const double v = (double)b / (double)(a != 0 ? a : 1);
    return (a != 0 && v > 0.2) ? v : 0.2;
}

// R6 from the per-bin inlier counts cnt[j * stride]: the score; *t_out = sum p[j] * binp[j] (R7)
__device__ __forceinline__ double grid_score(const uint16_t* cnt, int stride, const int* start, const double* binp, int gr, int gc, double* t_out) {
    double S = 0.0, Q = 0.0, wx = 0.0, wy = 0.0, t = 0.0;
    for (int j = 0; j < GRID; ++j) {
        const double p = grid_p((int)cnt[j * stride], start[j + 1] - start[j]);
        const double cx = (double)(gr * (j / 10) + gr / 2), cy = (double)(gc * (j % 10) + gc / 2);
        S = S + p; Q = Q + p * p; wx = wx + p * cx; wy = wy + p * cy;
        t = t + p * binp[j];
    }
    const double mx = wx / S, my = wy / S;
    double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
    for (int j = 0; j < GRID; ++j) {
        const double p = grid_p((int)cnt[j * stride], start[j + 1] - start[j]);
        const double cx = (double)(gr * (j / 10) + gr / 2), cy = (double)(gc * (j % 10) + gc / 2);
        const double dx = cx - mx, dy = cy - my, px = p * dx, py = p * dy;
        c00 = c00 + px * dx; c01 = c01 + px * dy; c10 = c10 + py * dx; c11 = c11 + py * dy;
    }
    const double den = S * S - Q;
    c00 = (c00 * S) / den; c01 = (c01 * S) / den; c10 = (c10 * S) / den; c11 = (c11 * S) / den;
    const double det = c00 * c11 - c10 * c01;
    *t_out = t;
    return (S * 3.14159265358979323846) * sqrt(det);
}

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&G)[3][3], double (&V)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = G[P][Q];
    if (apq != 0.0) {
        const double theta = (G[Q][Q] - G[P][P]) / (2.0 * apq);
        const double den = fabs(theta) + sqrt(theta * theta + 1.0);
        const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        G[P][P] = G[P][P] - t * apq; G[Q][Q] = G[Q][Q] + t * apq;
        G[P][Q] = 0.0; G[Q][P] = 0.0;
        const double grp = G[R][P], grq = G[R][Q];
        G[R][P] = c * grp - s * grq; G[P][R] = G[R][P];
        G[R][Q] = s * grp + c * grq; G[Q][R] = G[R][Q];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vp = V[k][P], vq = V[k][Q];
            V[k][P] = c * vp - s * vq;
            V[k][Q] = s * vp + c * vq;
        }
    }
}

// R4 for the eight correspondences p[0..8): the float32 F; false when the hypothesis is invalid
__device__ __forceinline__ bool solve8(const float4 (&p)[8], float (&Fout)[9]) {
    double m1x = 0.0, m1y = 0.0, m2x = 0.0, m2y = 0.0, d1x = 0.0, d1y = 0.0, d2x = 0.0, d2y = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) { m1x = m1x + (double)p[s].x / 8.0; m1y = m1y + (double)p[s].y / 8.0; m2x = m2x + (double)p[s].z / 8.0; m2y = m2y + (double)p[s].w / 8.0; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        d1x = d1x + fabs((double)p[s].x - m1x) / 8.0; d1y = d1y + fabs((double)p[s].y - m1y) / 8.0;
        d2x = d2x + fabs((double)p[s].z - m2x) / 8.0; d2y = d2y + fabs((double)p[s].w - m2y) / 8.0;
    }
    const double s1x = 1.0 / d1x, s1y = 1.0 / d1y, s2x = 1.0 / d2x, s2y = 1.0 / d2y;
    double A[8][9], amax = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const double u1 = s1x * ((double)p[s].x - m1x), v1 = s1y * ((double)p[s].y - m1y);
        const double u2 = s2x * ((double)p[s].z - m2x), v2 = s2y * ((double)p[s].w - m2y);
        A[s][0] = u2 * u1; A[s][1] = u2 * v1; A[s][2] = u2; A[s][3] = v2 * u1; A[s][4] = v2 * v1; A[s][5] = v2; A[s][6] = u1; A[s][7] = v1; A[s][8] = 1.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) amax = fabs(A[s][j]) > amax ? fabs(A[s][j]) : amax;
    }
    // the elimination: rows and columns keep their places and a used row stays in A as it was when it gave the pivot; the pivot row and
    // the pivot column's entries are picked out by select chains (no dynamic index: nothing goes to scratch)
    double last = 0.0;
    int colstep[9], rowstep[8];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) colstep[j] = 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) rowstep[i] = -1;
#pragma unroll 1
    for (int s = 0; s < 8; ++s) {
        double best = -1.0;
        int pr = 0, pc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double mag = fabs(A[i][j]);
                const bool take = rowstep[i] < 0 && colstep[j] == 8 && mag > best;
                best = take ? mag : best; pr = take ? i : pr; pc = take ? j : pc;
            }
        ok = ok && !(best < 0.0);
        double Rs[9], pv = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double v = A[0][j];
#pragma unroll
            for (int i = 1; i < 8; ++i) v = pr == i ? A[i][j] : v;
            Rs[j] = v;
            pv = pc == j ? v : pv;
        }
        last = best;
#pragma unroll
        for (int i = 0; i < 8; ++i) rowstep[i] = pr == i ? s : rowstep[i];
#pragma unroll
        for (int j = 0; j < 9; ++j) colstep[j] = pc == j ? s : colstep[j];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double e = A[i][0];
#pragma unroll
            for (int j = 1; j < 9; ++j) e = pc == j ? A[i][j] : e;
            const double f = e / pv;
            const bool used = rowstep[i] >= 0;
#pragma unroll
            for (int j = 0; j < 9; ++j) A[i][j] = used ? A[i][j] : A[i][j] - f * Rs[j];
        }
    }
    ok = ok && last > 1e-12 * amax;
    double x[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) x[j] = colstep[j] == 8 ? 1.0 : 0.0;
#pragma unroll
    for (int s = 7; s >= 0; --s) {
        double acc = 0.0, pv = 1.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double v = A[0][j];
#pragma unroll
            for (int i = 1; i < 8; ++i) v = rowstep[i] == s ? A[i][j] : v;
            acc = colstep[j] > s ? acc + v * x[j] : acc;
            pv = colstep[j] == s ? v : pv;
        }
        const double xs = (0.0 - acc) / pv;
#pragma unroll
        for (int j = 0; j < 9; ++j) x[j] = colstep[j] == s ? xs : x[j];
    }
    double n2 = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) n2 = n2 + x[j] * x[j];
    const double nrm = sqrt(n2);
    double F[3][3];
#pragma unroll
    for (int j = 0; j < 9; ++j) F[j / 3][j % 3] = x[j] / nrm;
    double G[3][3], V[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) { G[a][b] = (F[0][a] * F[0][b] + F[1][a] * F[1][b]) + F[2][a] * F[2][b]; V[a][b] = a == b ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) { jacobi_rotate<0, 1>(G, V); jacobi_rotate<0, 2>(G, V); jacobi_rotate<1, 2>(G, V); }
    int e = 0;
    double ge = G[0][0];
    if (G[1][1] < ge) { e = 1; ge = G[1][1]; }
    if (G[2][2] < ge) { e = 2; ge = G[2][2]; }
    double w0 = e == 0 ? V[0][0] : (e == 1 ? V[0][1] : V[0][2]);
    double w1 = e == 0 ? V[1][0] : (e == 1 ? V[1][1] : V[1][2]);
    double w2 = e == 0 ? V[2][0] : (e == 1 ? V[2][1] : V[2][2]);
    const double vn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double v[3] = {w0 / vn, w1 / vn, w2 / vn};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double w = (F[r][0] * v[0] + F[r][1] * v[1]) + F[r][2] * v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) F[r][c] = F[r][c] - w * v[c];
    }
    const double t1x = -(m1x * s1x), t1y = -(m1y * s1y), t2x = -(m2x * s2x), t2y = -(m2y * s2y);
    double Pm[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Pm[0][c] = s2x * F[0][c];
        Pm[1][c] = s2y * F[1][c];
        Pm[2][c] = (t2x * F[0][c] + t2y * F[1][c]) + F[2][c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double q[3] = {Pm[r][0] * s1x, Pm[r][1] * s1y, (Pm[r][0] * t1x + Pm[r][1] * t1y) + Pm[r][2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = (float)q[c];
            ok = ok && (f - f) == 0.0f;
            Fout[3 * r + c] = f;
        }
    }
    return ok;
}

__global__ __launch_bounds__(THREADS) void rarsac_kernel(const RarsacDev* __restrict__ recs) {
    __shared__ float4 s_pt[MAX_POINTS];                     // 32 KB
    __shared__ uint16_t s_cnt[GRID * THREADS];              // 50 KB: a lane's inliers per bin, [bin][lane]
    __shared__ double s_score[THREADS], s_q[THREADS], s_binp[GRID];
    __shared__ int s_start[GRID + 1], s_nbin[GRID], s_cum[GRID];
    __shared__ uint16_t s_b[GRID];
    __shared__ uint8_t s_valid[THREADS];
    __shared__ float s_bestF[9];
    __shared__ double s_best, s_qcur, s_prod;
    __shared__ int s_bestk, s_run, s_stop, s_winner;

    const RarsacDev r = recs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    // (the host checked them; they bound the LDS arrays and the loops here)
    const int m = min(max(r.m, 0), MAX_POINTS), nb = min(max(r.nb, 0), GRID), max_iter = min(r.max_iterations, DSDTM_RARSAC_MAX_ITERATIONS);
    dsdtm_rarsac_result* __restrict__ out = r.out;
    if (!r.check && nb < 8) {                               // R3: fewer than 8 non-empty bins
        if (tid == 0) out->found = 0;
        return;
    }
    for (int i = tid; i < m; i += THREADS) s_pt[i] = ((const float4*)r.pt)[i];
    if (tid < GRID) {
        s_binp[tid] = r.table->binp[tid];
        s_nbin[tid] = min(max(r.table->nbin[tid], 0), GRID - 1);
        s_cum[tid] = r.table->cum[tid];
        s_b[tid] = 0;
    }
    if (tid <= GRID) s_start[tid] = min(max(r.table->start[tid], 0), m);
    if (tid == 0) { s_best = DBL_MIN_; s_qcur = 0.0; s_prod = 1.0; s_bestk = -1; s_run = 0; s_stop = 0; s_winner = -1; }
    if (tid < 9) s_bestF[tid] = r.check ? r.F[tid] : 0.0f;
    __syncthreads();

    const float inv_sigma2 = r.inv_sigma2;
    const int rounds = r.check ? 0 : (max_iter + THREADS - 1) / THREADS;
    for (int round = 0; round < rounds; ++round) {
        const int k = round * THREADS + tid;
        // R3: eight distinct non-empty bins by inverse CDF, a repeated bin redrawn with the next counter
        int ch[8] = {0, 0, 0, 0, 0, 0, 0, 0}, got = 0;
        for (uint32_t c = 0; c < (uint32_t)BIN_DRAWS; ++c) {
            if (got >= 8) break;
            const int t = (int)__umulhi(hash3(r.seed, (uint32_t)k, c), (uint32_t)r.total);
            int lo = 0, hi = nb - 1;
#pragma unroll
            for (int step = 0; step < 7; ++step) {
                const int mid = (lo + hi) >> 1;
                const bool right = lo < hi && s_cum[mid] <= t;
                const bool left = lo < hi && !right;
                lo = right ? mid + 1 : lo;
                hi = left ? mid : hi;
            }
            bool fresh = true;
#pragma unroll
            for (int s = 0; s < 8; ++s) fresh = fresh && !(s < got && ch[s] == lo);
#pragma unroll
            for (int s = 0; s < 8; ++s) ch[s] = (fresh && got == s) ? lo : ch[s];
            got += fresh ? 1 : 0;
        }
        float4 p[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int bin = s_nbin[ch[s]], first = s_start[bin], count = s_start[bin + 1] - first;
            const int at = first + (int)__umulhi(hash3(r.seed, (uint32_t)k, (uint32_t)(BIN_DRAWS + s)), (uint32_t)count);
            p[s] = s_pt[min(at, MAX_POINTS - 1)];
        }
        float F[9];
        const bool valid = solve8(p, F) && got == 8 && k < max_iter;
        // R5: the walk in bin order, one running counter
        for (int j = 0; j < GRID; ++j) {
            int cnt = 0;
            const int end = s_start[j + 1];
            for (int i = s_start[j]; i < end; ++i) cnt += inlier(F, s_pt[i], inv_sigma2);
            s_cnt[j * THREADS + tid] = (uint16_t)cnt;
        }
        double t = 0.0;
        const double score = grid_score(&s_cnt[tid], THREADS, s_start, s_binp, r.gr, r.gc, &t);
        const double t2 = t * t, t4 = t2 * t2, t8 = t4 * t4;
        s_score[tid] = score; s_q[tid] = 1.0 - t8; s_valid[tid] = valid ? 1 : 0;
        __syncthreads();
        if (tid == 0) {                                     // R7-R9: the ordered scan
            double best = s_best, q = s_qcur, prod = s_prod;
            int bestk = s_bestk, run = s_run, stop = 0, winner = -1;
            for (int l = 0; l < THREADS; ++l) {
                const int kk = round * THREADS + l;
                if (kk >= max_iter) break;
                run = kk + 1;
                if (!s_valid[l]) continue;
                const double sc = s_score[l];
                if (sc > best) { best = sc; bestk = kk; winner = l; q = s_q[l]; prod = 1.0; }
                prod = prod * q;
                if ((double)(float)prod < r.terminate) { stop = 1; break; }
            }
            s_best = best; s_qcur = q; s_prod = prod; s_bestk = bestk; s_run = run; s_stop = stop; s_winner = winner;
        }
        __syncthreads();
        if (s_winner == tid) {
#pragma unroll
            for (int j = 0; j < 9; ++j) s_bestF[j] = F[j];
        }
        __syncthreads();
        if (s_stop) break;
    }

    const bool have = r.check || s_bestk >= 0;
    if (have) {                                             // the winner's status and counts, recomputed: thread j owns bin j
        float F[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) F[j] = s_bestF[j];
        if (tid < GRID) {
            int cnt = 0;
            const int end = s_start[tid + 1];
            for (int i = s_start[tid]; i < end; ++i) {
                const int in = inlier(F, s_pt[i], inv_sigma2);
                r.status[i] = (uint8_t)in;
                cnt += in;
            }
            s_b[tid] = (uint16_t)cnt;
        }
    } else {
        for (int i = tid; i < m; i += THREADS) r.status[i] = 0;
    }
    __syncthreads();
    if (tid < GRID) out->grid_probability_out[tid] = have ? grid_p((int)s_b[tid], s_start[tid + 1] - s_start[tid]) : r.table->prior[tid];
    if (tid == 0) {
        double t = 0.0;
        const double sc = grid_score(s_b, 1, s_start, s_binp, r.gr, r.gc, &t);
        int n_in = 0;
        for (int j = 0; j < GRID; ++j) n_in += (int)s_b[j];
        out->score = r.check ? sc : s_best;
#pragma unroll
        for (int j = 0; j < 9; ++j) out->F[j] = s_bestF[j];
        out->found = 1; out->best_hypothesis = s_bestk; out->iterations_run = s_run; out->n_inliers = n_in;
        out->reserved[0] = 0; out->reserved[1] = 0; out->reserved[2] = 0;
    }
}

}  // namespace

hipError_t rarsac_launch(const RarsacDev* recs, int n, hipStream_t stream) {
    hipLaunchKernelGGL(rarsac_kernel, dim3((unsigned)n), dim3(THREADS), 0, stream, recs);
    return hipGetLastError();
}

}  // namespace dsdtm
