// dsdtm_rarsac_host.hpp — Rarsac_base::RejectFundamental (src/Rarsac_base.cpp of the reference): the grid-guided RANSAC for the
// fundamental matrix that rejects outliers among frame-to-frame correspondences and updates the frame's 10x10 inlier-probability grid.
// Header-only; needs neither OpenCV nor Eigen.
//
//   reject_fundamental_host / check_fundamental_host   rules R1-R9 of include/dsdtm_amd_rarsac.h on ONE HOST THREAD, no library needed;
//                                                      bit-equal to dsdtm_amd/rarsac_restatement.py and to the device.
//   DSDTM::Rarsac_base(grid, pts1, pts2)               the reference's class: RejectFundamental() returns the status vector and writes
//                                                      the frame's grid back (src/Rarsac_base.cpp:250). The pipeline it belongs to
//                                                      (Test/test_Optimizer.cpp:91-106): dsdtm_klt_flow, then this, then ReduceFeatures.
//   dsdtm_rarsac_reject_batch (the C header)           n trackers in one submission: what the device is for.
//
// PARITY: which samples are drawn and how the 8-point system is solved are this project's definition (cv::SVDecomp and
// std::random_shuffle cannot be restated, and the reference's sampling loop reads past mvBinIndexProba); the scoring, the grid update,
// the best-so-far rule and the stop rule follow the reference operation by operation. Parity with OpenCV is unpinned.
//
// WHICH PATH. Measured on one MI355X at 300 correspondences (profiles/r26_rarsac.txt, wall per call): one problem takes the device
// 199 us with clean matches (about 150 hypotheses: one round) and 721 us with 40 % outliers (all 1000 hypotheses: four rounds), against
// 562 us and 2837 us for reject_fundamental_host on one host thread; in a batch the device needs 7-13 us per problem at n = 64 and
// 2.4-4.2 us at n = 1024. The host function wins nowhere measured, so Rarsac_base calls the DEVICE by default; on_device = false is for a
// machine without one. (Rarsac_base creates a context per call, which the figures above do not include: a process that calls it per
// frame should keep a dsdtm_rarsac_ctx and call dsdtm_rarsac_reject, or collect its trackers into ONE dsdtm_rarsac_reject_batch.)
// Compile with -ffp-contract=off (the arithmetic is one order of + - * / sqrt without contraction). -DDSDTM_RARSAC_HOST_ONLY leaves out
// everything that needs the library.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_rarsac.h"

namespace dsdtm {
namespace rarsac_detail {

constexpr int GRID = DSDTM_RARSAC_GRID;
constexpr int MAX_POINTS = DSDTM_RARSAC_MAX_POINTS;
constexpr int BIN_DRAWS = 64;
constexpr int JACOBI_SWEEPS = 8;

struct problem {
    int m, nb, gr, gc, total;
    int start[GRID + 1], a[GRID], nbin[GRID], cum[GRID];
    double binp[GRID], cx[GRID], cy[GRID];
    float inv_sigma2;
    uint32_t seed;
    int order[MAX_POINTS];          /* sorted position -> correspondence */
    float pt[MAX_POINTS][4];        /* sorted by bin: cur x, cur y, prev x, prev y */
    int bins[MAX_POINTS];
    uint8_t sorted[MAX_POINTS];
};

inline uint32_t hash3(uint32_t seed, uint32_t k, uint32_t c) {
    uint32_t x = seed + k * 0x9E3779B9u + c * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
inline uint32_t mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
inline int finite_d(double v) { return (v - v) == 0.0; }

/* R1: the bin of a point, or -1 */
inline int bin_of(float x, float y, int gr, int gc) {
    const float r = y / (float)gc, c = x / (float)gr;
    if (!(r > -1000000.0f && r < 1000000.0f && c > -1000000.0f && c < 1000000.0f)) return -1;
    const int idx = (int)r * 10 + (int)c;
    return idx < 0 || idx >= GRID ? -1 : idx;
}

/* R1-R3 set-up. Returns 0, or -(1 + index) for a correspondence that R1 refuses. */
inline int set_up(problem* P, const float* cur, const float* prev, int m, int width, int height, const double* prior, float sigma, uint32_t seed) {
    int* bins = P->bins;
    int fill[GRID];
    P->m = m; P->gr = height / 10; P->gc = width / 10; P->seed = seed;
    memset(P->a, 0, sizeof P->a);
    for (int i = 0; i < m; ++i) {
        const int ok = finite_d((double)cur[2 * i]) && finite_d((double)cur[2 * i + 1]) && finite_d((double)prev[2 * i]) && finite_d((double)prev[2 * i + 1]);
        const int b = ok ? bin_of(cur[2 * i], cur[2 * i + 1], P->gr, P->gc) : -1;
        if (b < 0) return -(1 + i);
        bins[i] = b;
        P->a[b]++;
    }
    P->start[0] = 0;
    for (int j = 0; j < GRID; ++j) { P->start[j + 1] = P->start[j] + P->a[j]; fill[j] = P->start[j]; }
    for (int i = 0; i < m; ++i) {
        const int at = fill[bins[i]]++;
        P->order[at] = i;
        P->pt[at][0] = cur[2 * i]; P->pt[at][1] = cur[2 * i + 1]; P->pt[at][2] = prev[2 * i]; P->pt[at][3] = prev[2 * i + 1];
    }
    double sum = 0.0;
    for (int j = 0; j < GRID; ++j) sum = sum + prior[j];
    P->nb = 0; P->total = 0;
    for (int j = 0; j < GRID; ++j) {
        P->binp[j] = prior[j] / sum;
        P->cx[j] = (double)(P->gr * (j / 10) + P->gr / 2);
        P->cy[j] = (double)(P->gc * (j % 10) + P->gc / 2);
        if (P->a[j] > 0) {
            int w = (int)(prior[j] * 1024.0);
            if (w < 1) w = 1;
            P->total += w;
            P->nbin[P->nb] = j; P->cum[P->nb] = P->total;
            P->nb++;
        }
    }
    const float s2 = sigma * sigma;
    P->inv_sigma2 = (float)(1.0 / (double)s2);
    return 0;
}

/* R3: the eight sorted positions of hypothesis k; 0 when 64 draws did not give 8 distinct bins */
inline int draw_sample(const problem* P, uint32_t k, int* at) {
    int chosen[8], got = 0;
    for (uint32_t c = 0; c < BIN_DRAWS && got < 8; ++c) {
        const uint32_t t = mulhi(hash3(P->seed, k, c), (uint32_t)P->total);
        int i = 0;
        while (P->cum[i] <= (int)t) ++i;
        int fresh = 1;
        for (int s = 0; s < got; ++s) fresh = fresh && chosen[s] != i;
        if (fresh) chosen[got++] = i;
    }
    if (got < 8) return 0;
    for (int s = 0; s < 8; ++s) {
        const int bin = P->nbin[chosen[s]];
        at[s] = P->start[bin] + (int)mulhi(hash3(P->seed, k, (uint32_t)(BIN_DRAWS + s)), (uint32_t)P->a[bin]);
    }
    return 1;
}

/* R4: mean, mean absolute deviation and scales of eight coordinates pairs (columns o, o + 1 of the sample) */
inline void normalise8(const problem* P, const int* at, int o, double* mx, double* my, double* sx, double* sy) {
    double ax = 0.0, ay = 0.0, dx = 0.0, dy = 0.0;
    for (int s = 0; s < 8; ++s) { ax = ax + (double)P->pt[at[s]][o] / 8.0; ay = ay + (double)P->pt[at[s]][o + 1] / 8.0; }
    for (int s = 0; s < 8; ++s) { dx = dx + fabs((double)P->pt[at[s]][o] - ax) / 8.0; dy = dy + fabs((double)P->pt[at[s]][o + 1] - ay) / 8.0; }
    *mx = ax; *my = ay; *sx = 1.0 / dx; *sy = 1.0 / dy;
}

inline void jacobi_rotate(double G[3][3], double V[3][3], int p, int q) {
    const double apq = G[p][q];
    if (apq == 0.0) return;
    const int r = 3 - p - q;
    const double theta = (G[q][q] - G[p][p]) / (2.0 * apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    G[p][p] = G[p][p] - t * apq; G[q][q] = G[q][q] + t * apq;
    G[p][q] = 0.0; G[q][p] = 0.0;
    const double grp = G[r][p], grq = G[r][q];
    G[r][p] = c * grp - s * grq; G[p][r] = G[r][p];
    G[r][q] = s * grp + c * grq; G[q][r] = G[r][q];
    for (int k = 0; k < 3; ++k) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = c * vp - s * vq;
        V[k][q] = s * vp + c * vq;
    }
}

/* R4: the float32 F of the sample; 0 when the hypothesis is invalid */
inline int solve8(const problem* P, const int* at, float* Fout) {
    double m1x, m1y, s1x, s1y, m2x, m2y, s2x, s2y;
    normalise8(P, at, 0, &m1x, &m1y, &s1x, &s1y);
    normalise8(P, at, 2, &m2x, &m2y, &s2x, &s2y);
    double A[8][9], amax = 0.0;
    for (int s = 0; s < 8; ++s) {
        const float* p = P->pt[at[s]];
        const double u1 = s1x * ((double)p[0] - m1x), v1 = s1y * ((double)p[1] - m1y);
        const double u2 = s2x * ((double)p[2] - m2x), v2 = s2y * ((double)p[3] - m2y);
        const double row[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
        for (int j = 0; j < 9; ++j) { A[s][j] = row[j]; if (fabs(row[j]) > amax) amax = fabs(row[j]); }
    }
    double R[8][9], piv[8], last = 0.0;
    int rowstep[8], colstep[9];
    for (int i = 0; i < 8; ++i) rowstep[i] = -1;
    for (int j = 0; j < 9; ++j) colstep[j] = 8;
    for (int s = 0; s < 8; ++s) {
        double best = -1.0;
        int pr = 0, pc = 0;
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 9; ++j)
                if (rowstep[i] < 0 && colstep[j] == 8 && fabs(A[i][j]) > best) { best = fabs(A[i][j]); pr = i; pc = j; }
        if (best < 0.0) return 0;                       /* nothing but NaN is left */
        const double pv = A[pr][pc];
        for (int j = 0; j < 9; ++j) R[s][j] = A[pr][j];
        piv[s] = pv; last = best;
        rowstep[pr] = s; colstep[pc] = s;
        for (int i = 0; i < 8; ++i) {
            if (rowstep[i] >= 0) continue;
            const double f = A[i][pc] / pv;
            for (int j = 0; j < 9; ++j) A[i][j] = A[i][j] - f * R[s][j];
        }
    }
    if (!(last > 1e-12 * amax)) return 0;
    double x[9];
    for (int j = 0; j < 9; ++j) x[j] = colstep[j] == 8 ? 1.0 : 0.0;
    for (int s = 7; s >= 0; --s) {
        double acc = 0.0;
        int pc = 0;
        for (int j = 0; j < 9; ++j) {
            if (colstep[j] > s) acc = acc + R[s][j] * x[j];
            if (colstep[j] == s) pc = j;
        }
        x[pc] = (0.0 - acc) / piv[s];
    }
    double n2 = 0.0;
    for (int j = 0; j < 9; ++j) n2 = n2 + x[j] * x[j];
    const double nrm = sqrt(n2);
    double F[3][3];
    for (int j = 0; j < 9; ++j) F[j / 3][j % 3] = x[j] / nrm;
    /* rank 2 */
    double G[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) G[a][b] = (F[0][a] * F[0][b] + F[1][a] * F[1][b]) + F[2][a] * F[2][b];
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) { jacobi_rotate(G, V, 0, 1); jacobi_rotate(G, V, 0, 2); jacobi_rotate(G, V, 1, 2); }
    int e = 0;
    if (G[1][1] < G[e][e]) e = 1;
    if (G[2][2] < G[e][e]) e = 2;
    const double vn = sqrt((V[0][e] * V[0][e] + V[1][e] * V[1][e]) + V[2][e] * V[2][e]);
    const double v[3] = {V[0][e] / vn, V[1][e] / vn, V[2][e] / vn};
    for (int r = 0; r < 3; ++r) {
        const double w = (F[r][0] * v[0] + F[r][1] * v[1]) + F[r][2] * v[2];
        for (int c = 0; c < 3; ++c) F[r][c] = F[r][c] - w * v[c];
    }
    /* T2^T F T1 */
    const double t1x = -(m1x * s1x), t1y = -(m1y * s1y), t2x = -(m2x * s2x), t2y = -(m2y * s2y);
    double Pm[3][3];
    for (int c = 0; c < 3; ++c) {
        Pm[0][c] = s2x * F[0][c];
        Pm[1][c] = s2y * F[1][c];
        Pm[2][c] = (t2x * F[0][c] + t2y * F[1][c]) + F[2][c];
    }
    int ok = 1;
    for (int r = 0; r < 3; ++r) {
        const double q[3] = {Pm[r][0] * s1x, Pm[r][1] * s1y, (Pm[r][0] * t1x + Pm[r][1] * t1y) + Pm[r][2]};
        for (int c = 0; c < 3; ++c) {
            const float f = (float)q[c];
            ok = ok && (f - f) == 0.0f;
            Fout[3 * r + c] = f;
        }
    }
    return ok;
}

/* R5: whether the correspondence at a sorted position is an inlier of F */
inline int inlier(const float* F, const float* p, float inv_sigma2) {
    const float th = 3.841f;
    const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
    int in = 1;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float d1 = (num2 * num2) / (a2 * a2 + b2 * b2);
    const float chi1 = d1 * inv_sigma2;
    if (chi1 > th) in = 0;
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float d2 = (num1 * num1) / (a1 * a1 + b1 * b1);
    const float chi2 = d2 * inv_sigma2;
    if (chi2 > th) in = 0;
    return in;
}

/* R5-R6: the grid p[100] and the score of F; status (sorted positions) when wanted */
inline double check_F(const problem* P, const float* F, double* p, uint8_t* status_sorted) {
    for (int j = 0; j < GRID; ++j) {
        int b = 0;
        for (int i = P->start[j]; i < P->start[j + 1]; ++i) {
            const int in = inlier(F, P->pt[i], P->inv_sigma2);
            if (status_sorted) status_sorted[i] = (uint8_t)in;
            b += in;
        }
        p[j] = 0.2;
        if (P->a[j] != 0) { const double v = (double)b / (double)P->a[j]; p[j] = v > 0.2 ? v : 0.2; }
    }
    double S = 0.0, Q = 0.0, wx = 0.0, wy = 0.0;
    for (int j = 0; j < GRID; ++j) { S = S + p[j]; Q = Q + p[j] * p[j]; wx = wx + p[j] * P->cx[j]; wy = wy + p[j] * P->cy[j]; }
    const double mx = wx / S, my = wy / S;
    double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
    for (int j = 0; j < GRID; ++j) {
        const double dx = P->cx[j] - mx, dy = P->cy[j] - my, px = p[j] * dx, py = p[j] * dy;
        c00 = c00 + px * dx; c01 = c01 + px * dy; c10 = c10 + py * dx; c11 = c11 + py * dy;
    }
    const double den = S * S - Q;
    c00 = (c00 * S) / den; c01 = (c01 * S) / den; c10 = (c10 * S) / den; c11 = (c11 * S) / den;
    const double det = c00 * c11 - c10 * c01;
    return (S * 3.14159265358979323846) * sqrt(det);
}

}  // namespace rarsac_detail

/* R1-R9 on one host thread. Returns found (1 / 0; with 0 nothing is written) or -(1 + index) for a correspondence that R1 refuses.
 * The arguments are the desc's fields with the defaults filled in (8 <= m <= 2048, width and height at least 10, prior[100] in 0..1
 * with a positive sum: the caller's to guarantee). ints: best_hypothesis, iterations_run, n_inliers. */
inline int reject_fundamental_host(const float* cur, const float* prev, int m, int width, int height, const double* prior, int max_iterations, double terminate,
                                   float sigma, uint32_t seed, uint8_t* status, float* F, double* grid_out, double* score, int* ints) {
    using namespace rarsac_detail;
    problem* P = (problem*)malloc(sizeof(problem));
    if (!P) throw std::bad_alloc();
    const int bad = set_up(P, cur, prev, m, width, height, prior, sigma, seed);
    if (bad < 0 || P->nb < 8) { const int nb_short = bad >= 0; free(P); return nb_short ? 0 : bad; }
    double best = DBL_MIN, q = 0.0, prod = 1.0, p[GRID], bestp[GRID];
    float bestF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Fk[9];
    int best_k = -1, run = 0;
    for (int j = 0; j < GRID; ++j) bestp[j] = prior[j];
    for (int k = 0; k < max_iterations; ++k) {
        int at[8];
        run = k + 1;
        if (!draw_sample(P, (uint32_t)k, at) || !solve8(P, at, Fk)) continue;
        const double sc = check_F(P, Fk, p, NULL);
        if (sc > best) {
            best = sc; best_k = k;
            memcpy(bestF, Fk, sizeof bestF); memcpy(bestp, p, sizeof bestp);
            double t = 0.0;
            for (int j = 0; j < GRID; ++j) t = t + p[j] * P->binp[j];
            const double t2 = t * t, t4 = t2 * t2, t8 = t4 * t4;
            q = 1.0 - t8;
            prod = 1.0;
        }
        prod = prod * q;
        if ((double)(float)prod < terminate) break;
    }
    uint8_t* sorted = P->sorted;
    int n_in = 0;
    memset(sorted, 0, MAX_POINTS);
    if (best_k >= 0) (void)check_F(P, bestF, p, sorted);
    for (int i = 0; i < m; ++i) { status[P->order[i]] = sorted[i]; n_in += sorted[i]; }
    memcpy(F, bestF, sizeof bestF); memcpy(grid_out, bestp, sizeof bestp);
    *score = best; ints[0] = best_k; ints[1] = run; ints[2] = n_in;
    free(P);
    return 1;
}

/* R5-R6 for a caller's F (the stateless CheckFundamental). Returns 1, or -(1 + index). ints: n_inliers. */
inline int check_fundamental_host(const float* cur, const float* prev, int m, int width, int height, const float* F, float sigma, uint8_t* status,
                                  double* grid_out, double* score, int* ints) {
    using namespace rarsac_detail;
    problem* P = (problem*)malloc(sizeof(problem));
    if (!P) throw std::bad_alloc();
    double prior[GRID], p[GRID];
    for (int j = 0; j < GRID; ++j) prior[j] = 0.5;
    const int bad = set_up(P, cur, prev, m, width, height, prior, sigma, 0u);
    if (bad < 0) { free(P); return bad; }
    uint8_t* sorted = P->sorted;
    int n_in = 0;
    *score = check_F(P, F, p, sorted);
    for (int i = 0; i < m; ++i) { status[P->order[i]] = sorted[i]; n_in += sorted[i]; }
    memcpy(grid_out, p, sizeof p);
    ints[0] = n_in;
    free(P);
    return 1;
}

}  // namespace dsdtm

namespace DSDTM {

struct RarsacPoint2f { float x, y; };                    // cv::Point2f

// The reference's class over this project's definition. `frame_grid_probability` is Frame::mvGrid_probability (100 doubles; Reset_Gridproba
// gives 0.5): RejectFundamental() returns the status vector (1 = consistent with the winning F) and, when a hypothesis won, writes the
// grid back as src/Rarsac_base.cpp:250 does. With fewer than 8 occupied bins it returns an empty vector and leaves the grid alone.
// on_device = true (the default, see WHICH PATH above) calls libdsdtm_amd_rarsac.so; false runs reject_fundamental_host.
class Rarsac_base {
public:
    Rarsac_base(std::vector<double>& frame_grid_probability, const std::vector<RarsacPoint2f>& pts1, const std::vector<RarsacPoint2f>& pts2, int width = 640,
                int height = 480, bool on_device = true, int device = 0)
        : grid_(frame_grid_probability), cur_(pts1), prev_(pts2), width_(width), height_(height), on_device_(on_device), device_(device) {
        if (pts1.size() != pts2.size()) throw std::runtime_error("Rarsac_base: pts1 and pts2 differ in length");
        if (grid_.size() != (size_t)DSDTM_RARSAC_GRID) throw std::runtime_error("Rarsac_base: the grid has not 100 entries");
    }

    std::vector<uint8_t> RejectFundamental() {
        const int m = (int)cur_.size();
        if (m < DSDTM_RARSAC_MIN_POINTS || m > DSDTM_RARSAC_MAX_POINTS) throw std::runtime_error("Rarsac_base: the number of correspondences is outside 8..2048");
        std::vector<uint8_t> status((size_t)m, 0);
        result = dsdtm_rarsac_result{};
        int found = 0;
        if (on_device_) {
#ifndef DSDTM_RARSAC_HOST_ONLY
            dsdtm_rarsac_ctx* ctx = nullptr;
            if (dsdtm_rarsac_create(device_, &ctx) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_rarsac_create: ") + dsdtm_rarsac_last_error(nullptr));
            const int rc = dsdtm_rarsac_reject(ctx, m, &cur_[0].x, &prev_[0].x, width_, height_, grid_.data(), status.data(), &result);
            const std::string why = rc == DSDTM_OK ? "" : dsdtm_rarsac_last_error(ctx);
            dsdtm_rarsac_destroy(ctx);
            if (rc != DSDTM_OK) throw std::runtime_error("dsdtm_rarsac_reject: " + why);
            found = result.found;
#else
            throw std::runtime_error("Rarsac_base: built with DSDTM_RARSAC_HOST_ONLY");
#endif
        } else {
            int ints[3] = {-1, 0, 0};
            found = dsdtm::reject_fundamental_host(&cur_[0].x, &prev_[0].x, m, width_, height_, grid_.data(), DSDTM_RARSAC_DEFAULT_ITERATIONS,
                                                   DSDTM_RARSAC_DEFAULT_TERMINATE, (float)DSDTM_RARSAC_DEFAULT_SIGMA, DSDTM_RARSAC_DEFAULT_SEED, status.data(),
                                                   result.F, result.grid_probability_out, &result.score, ints);
            if (found < 0) throw std::runtime_error("Rarsac_base: correspondence " + std::to_string(-found - 1) + " is refused by R1");
            result.found = found; result.best_hypothesis = ints[0]; result.iterations_run = ints[1]; result.n_inliers = ints[2];
        }
        if (found != 1) return {};
        if (result.best_hypothesis >= 0) grid_.assign(result.grid_probability_out, result.grid_probability_out + DSDTM_RARSAC_GRID);
        return status;
    }

    dsdtm_rarsac_result result{};          // of the last RejectFundamental

private:
    std::vector<double>& grid_;
    const std::vector<RarsacPoint2f>& cur_;
    const std::vector<RarsacPoint2f>& prev_;
    int width_, height_;
    bool on_device_;
    int device_;
};

// The caller's ReduceFeatures (Tracking::ReduceFeatures): keep what the status marks
template <class T>
inline void ReduceFeatures(std::vector<T>& v, const std::vector<uint8_t>& status) {
    size_t j = 0;
    for (size_t i = 0; i < v.size() && i < status.size(); ++i)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}

}  // namespace DSDTM
