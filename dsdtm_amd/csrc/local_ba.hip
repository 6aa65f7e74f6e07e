// local_ba.hip — Optimizer::LocalBundleAdjustment (reference src/Optimizer.cpp:103-282): the solve and the outlier pass.
//
// What the reference runs is a Ceres problem with one 6-parameter block [t, log R] per keyframe (fixed keyframes and
// mlId == 0 constant), one free 3-parameter block per local map point, a FullBA_Problem residual per observation
// (include/Optimizer.h:129-216), HuberLoss(delta), DENSE_SCHUR, at most 10 iterations. The minimiser is restated from
// Ceres 1.13 as for PoseOptimization (pose_opt.hip); what local BA adds: the points
// are the eliminated blocks, D^2 is added to every point's 3x3 block before it is inverted and to the reduced camera
// matrix, which is solved by Cholesky; the points come back by back-substitution; the model decrease is taken from J * step.
//
// Mapping: ONE WORKGROUP (256 threads) PER PROBLEM, the whole trust-region loop on the device. Passes, each a strided
// loop over its items between barriers:
//   observations : residual, 2x6 / 2x3 Jacobians, Huber weight (stored, Jacobi-scaled, in the workspace); J * step; cost
//   points       : V = sum Jp^T Jp + D^2, its inverse (3x3 Cholesky), F_i = W_i V^-1 per free observation; back-substitution
//   pose pairs   : one thread per block (a, b), a <= b, of the reduced camera matrix: - sum F_i W_j^T over the points a and
//                  b both observe, in point order (the pair lists are built once per problem: the topology never changes)
//   poses        : one thread per free keyframe: U_a, g_a, the right-hand side, Plus
//   reduced solve: <= 96 x 96 in LDS, right-looking Cholesky by the workgroup, substitutions by one wave
// Every sum has a fixed order (a thread's items in order, then a fixed LDS tree): a problem gives the same bits alone, in
// any batch and run after run. No floating-point atomics.
#include <hip/hip_runtime.h>
#include <float.h>

#include "device_math.h"
#include "kernels.h"
#include "pose_math.h"

namespace dsdtm {

namespace {

constexpr int NT = 256;                                           // threads per problem
constexpr int MAXF = DSDTM_LBA_MAX_FREE_KF;                       // pose blocks of the reduced camera matrix
constexpr int MAXK = DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF;
constexpr int MAXN = 6 * MAXF;
constexpr int MAXB = MAXF * (MAXF + 1) / 2;                       // upper blocks (a <= b)
constexpr int JS = 20;     // per observation: r'[2], Jc'[12] (row-major 2x6), Jp'[6] (2x3)
constexpr int FS = 18;     // per observation: F = W' V'^-1 (6x3)
constexpr int PS = 24;     // per point: cand[3] scale[3] diag[3] vinv[6] g'[3] step[3]
enum { P_CAND = 0, P_SCALE = 3, P_DIAG = 6, P_VINV = 9, P_G = 15, P_STEP = 18 };
constexpr int KF_THREAD0 = 160;                                   // threads [160, 160 + nf): the pose blocks; [0, nblk): pairs
static_assert(MAXB <= KF_THREAD0 && KF_THREAD0 + MAXF <= NT && MAXK <= NT, "thread roles overlap");

__host__ __device__ constexpr size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Ws {
    double* J; double* F; double* P; int32_t* pt_start; int32_t* table; int32_t* pairs;
};
__host__ __device__ inline size_t ws_layout(int n_pts, int n_obs, uint8_t* base, Ws* w) {
    const size_t N = (size_t)n_obs, NP = (size_t)n_pts;
    size_t o = 0;
    const size_t oJ = o; o += a256(N * JS * 8);
    const size_t oF = o; o += a256(N * FS * 8);
    const size_t oP = o; o += a256(NP * PS * 8);
    const size_t oS = o; o += a256((NP + 1) * 4);
    const size_t oT = o; o += a256(NP * MAXF * 4);
    const size_t oR = o; o += a256(N * 9 * 2 * 4);   // pairs: sum_p nf_p (nf_p + 1) / 2 <= 8.5 N (nf_p <= 16 distinct keyframes)
    if (w) {
        w->J = (double*)(base + oJ); w->F = (double*)(base + oF); w->P = (double*)(base + oP);
        w->pt_start = (int32_t*)(base + oS); w->table = (int32_t*)(base + oT); w->pairs = (int32_t*)(base + oR);
    }
    return o;
}

// pose_math.h (shared with pose_opt.hip): pose_of, so3_log, pose_plus; libm out of line (LAT = false), the register file
// of this kernel is full
constexpr bool LAT = false;

struct Shared {
    double S[MAXN * MAXN];                 // reduced camera matrix (full, symmetric), then its Cholesky factor (lower)
    double rhs[MAXN];                      // right-hand side of the reduced system
    double x[MAXK][6];                     // parameter blocks of every keyframe
    double T[MAXK][8];                     // pose_of(x): qw qx qy qz tx ty tz
    double R[MAXK][9];                     // its rotation matrix
    double xc[MAXF][6], Tc[MAXF][8];       // candidate of the free keyframes
    double kscale[MAXF][6], kdiag[MAXF][6], kg[MAXF][6], kstep[MAXF][6];
    double U[MAXF][21];
    double red[NT];
    int ired[NT];
    int slot[MAXK];                        // keyframe -> free slot (pose block), -1: constant / unobserved
    int slot_kf[MAXF];
    int pair_off[MAXB + 1];
    int nf;
};

__device__ __forceinline__ double block_sum(Shared& sh, double v) {
    const int tid = threadIdx.x;
    sh.red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sh.red[tid] += sh.red[tid + s];
        __syncthreads();
    }
    const double r = sh.red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_max(Shared& sh, double v) {
    const int tid = threadIdx.x;
    sh.red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sh.red[tid] = fmax(sh.red[tid], sh.red[tid + s]);
        __syncthreads();
    }
    const double r = sh.red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ int block_or(Shared& sh, int v) {
    const int tid = threadIdx.x;
    sh.ired[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sh.ired[tid] |= sh.ired[tid + s];
        __syncthreads();
    }
    const int r = sh.ired[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int sym3(int i, int j) {       // 3x3 upper: 00 01 02 11 12 22
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a == 0 ? b : (a == 1 ? 2 + b : 5);
}
__device__ __forceinline__ int sym6(int i, int j) {       // 6x6 upper, row-major
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a * 6 - a * (a - 1) / 2 + (b - a);
}

struct Prob {
    int K, NP, N;
    double* T_io; const uint8_t* kc; double* X;
    const int32_t* okf; const int32_t* opt; const double* bear; const int32_t* lev;
    uint8_t* outl;
    double delta;
};

// FullBA_Problem::Evaluate (include/Optimizer.h:139-197) of observation i at pose q (rotation Rm) and point Xp,
// HuberLoss + Ceres' corrector (rho'' <= 0: residual and Jacobians scaled by sqrt(rho')). Returns 1/2 rho.
template <bool JAC>
__device__ __forceinline__ double eval_obs(const Prob& p, int i, const double* q, const double* Rm, const double* Xp,
                                           double* out /* JS doubles, unscaled */) {
    const double b0 = p.bear[3 * (size_t)i], b1 = p.bear[3 * (size_t)i + 1], b2 = p.bear[3 * (size_t)i + 2];
    SE3d T;
    T.qw = q[0]; T.qx = q[1]; T.qy = q[2]; T.qz = q[3]; T.tx = q[4]; T.ty = q[5]; T.tz = q[6];
    double rx, ry, rz;
    quat_rotate(T, Xp[0], Xp[1], Xp[2], rx, ry, rz);
    const double px = rx + T.tx, py = ry + T.ty, pz = rz + T.tz;
    const double inv_scale = __hiloint2double((1023 - (p.lev[i] & 31)) << 20, 0);   // 1 / (1 << level), exact
    const double r0 = (b0 / b2 - px / pz) * inv_scale;
    const double r1 = (b1 / b2 - py / pz) * inv_scale;
    const double s = r0 * r0 + r1 * r1;
    const double bb = p.delta * p.delta;
    double rho, rho1;
    if (s > bb) {
        const double r = sqrt(s);
        rho = 2.0 * p.delta * r - bb;
        rho1 = fmax(DBL_MIN, p.delta / r);
    } else {
        rho = s; rho1 = 1.0;
    }
    if constexpr (JAC) {
        const double w = sqrt(rho1);
        const double zi = 1.0 / pz, zi2 = zi * zi;
        double J[12];
        J[0] = -zi; J[1] = 0.0; J[2] = px * zi2; J[3] = py * J[2]; J[4] = -(1.0 + px * J[2]); J[5] = py * zi;
        J[6] = 0.0; J[7] = -zi; J[8] = py * zi2; J[9] = 1.0 + py * J[8]; J[10] = -px * J[8]; J[11] = -px * zi;
        // Jp = -[zi, 0, -x zi2; 0, zi, -y zi2] R
        const double m02 = -px * zi2, m12 = -py * zi2;
        double Jp[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jp[c] = -(zi * Rm[c] + m02 * Rm[6 + c]);
            Jp[3 + c] = -(zi * Rm[3 + c] + m12 * Rm[6 + c]);
        }
        out[0] = r0 * w; out[1] = r1 * w;
#pragma unroll
        for (int k = 0; k < 12; ++k) out[2 + k] = J[k] * w;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[14 + k] = Jp[k] * w;
    }
    return 0.5 * rho;
}

__device__ __forceinline__ void set_pose(Shared& sh, int k, const double* x) {
    const SE3d T = pose_of<LAT>(x);
    sh.T[k][0] = T.qw; sh.T[k][1] = T.qx; sh.T[k][2] = T.qy; sh.T[k][3] = T.qz;
    sh.T[k][4] = T.tx; sh.T[k][5] = T.ty; sh.T[k][6] = T.tz;
    quat_to_matrix(T, sh.R[k]);
}

// One evaluation with Jacobians at the current parameters: J rows of every observation (weighted; Jacobi-scaled when
// `scaled`; the pose columns of a constant keyframe zero), returns the cost; *finite = every value finite.
__device__ double eval_all(Shared& sh, const Prob& p, const Ws& w, bool scaled, int* finite) {
    double part = 0.0;
    int ok = 1;
    for (int i = threadIdx.x; i < p.N; i += NT) {
        const int k = p.okf[i], q = p.opt[i];
        double* row = w.J + (size_t)i * JS;
        double out[JS];
        part += eval_obs<true>(p, i, sh.T[k], sh.R[k], p.X + 3 * (size_t)q, out);
        const int a = sh.slot[k];
        if (scaled) {
            const double* ps = w.P + (size_t)q * PS + P_SCALE;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int c = 0; c < 6; ++c) out[2 + 6 * r + c] = a >= 0 ? out[2 + 6 * r + c] * sh.kscale[a][c] : 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[14 + 3 * r + c] *= ps[c];
            }
        } else if (a < 0) {
#pragma unroll
            for (int c = 0; c < 12; ++c) out[2 + c] = 0.0;
        }
#pragma unroll
        for (int k2 = 0; k2 < JS; ++k2) {
            ok &= isfinite(out[k2]) ? 1 : 0;
            row[k2] = out[k2];
        }
    }
    __syncthreads();
    const double cost = block_sum(sh, part);
    *finite = !block_or(sh, ok ? 0 : 1) && isfinite(cost);
    return cost;
}

// Scaled gradient g' of every block (points: workspace, poses: sh.kg) and max |x - Plus(x, -g)| over the free blocks,
// g = g' / scale (the unscaled gradient the gradient test reads)
__device__ double gradient(Shared& sh, const Prob& p, const Ws& w) {
    double m = 0.0;
    for (int q = threadIdx.x; q < p.NP; q += NT) {
        const int i0 = w.pt_start[q], i1 = w.pt_start[q + 1];
        if (i0 == i1) continue;
        double g[3] = {0.0, 0.0, 0.0};
        for (int i = i0; i < i1; ++i) {
            const double* row = w.J + (size_t)i * JS;
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] += row[14 + c] * row[0] + row[17 + c] * row[1];
        }
        double* P = w.P + (size_t)q * PS;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[P_G + c] = g[c];
            const double x = p.X[3 * (size_t)q + c];
            m = fmax(m, fabs(x - (x + -(g[c] / P[P_SCALE + c]))));
        }
    }
    const int a = (int)threadIdx.x - KF_THREAD0;
    if (a >= 0 && a < sh.nf) {
        double g[6] = {0, 0, 0, 0, 0, 0};
        const int b = a * sh.nf - a * (a - 1) / 2;                // block (a, a): the observations of keyframe a
        for (int e = sh.pair_off[b]; e < sh.pair_off[b + 1]; ++e) {
            const double* row = w.J + (size_t)w.pairs[2 * (size_t)e] * JS;
#pragma unroll
            for (int c = 0; c < 6; ++c) g[c] += row[2 + c] * row[0] + row[8 + c] * row[1];
        }
        double gu[6], xn[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) { sh.kg[a][c] = g[c]; gu[c] = -(g[c] / sh.kscale[a][c]); }
        const double* x = sh.x[sh.slot_kf[a]];
        pose_plus<LAT>(pose_of<LAT>(x), gu, xn);
#pragma unroll
        for (int c = 0; c < 6; ++c) m = fmax(m, fabs(x[c] - xn[c]));
    }
    __syncthreads();
    return block_max(sh, m);
}

__device__ double x_norm(Shared& sh, const Prob& p, const Ws& w) {
    double s = 0.0;
    if ((int)threadIdx.x < sh.nf) {
        const double* x = sh.x[sh.slot_kf[threadIdx.x]];
#pragma unroll
        for (int c = 0; c < 6; ++c) s += x[c] * x[c];
    }
    for (int q = threadIdx.x; q < p.NP; q += NT)
        if (w.pt_start[q] != w.pt_start[q + 1]) {
            const double* X = p.X + 3 * (size_t)q;
            s += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
        }
    return sqrt(block_sum(sh, s));
}

// (a, b) of upper block bi of nf pose blocks, row-major
__device__ __forceinline__ void block_ab(int bi, int nf, int& a, int& b) {
    a = 0;
    while (bi >= nf - a) { bi -= nf - a; ++a; }
    b = a + bi;
}

__device__ void local_ba_body(const LocalBaArgs& args, Shared& sh) {
    const int tid = threadIdx.x;
    const LocalBaProblemDev D = args.problems[blockIdx.x];
    Prob p;
    p.K = D.n_kf; p.NP = D.n_pts; p.N = D.n_obs; p.delta = args.delta;
    p.T_io = args.T + 12 * D.kf_off; p.kc = args.kf_const + D.kf_off; p.X = args.points + 3 * D.pt_off;
    p.okf = args.obs_kf + D.obs_off; p.opt = args.obs_pt + D.obs_off; p.bear = args.bearing + 3 * D.obs_off;
    p.lev = args.level + D.obs_off; p.outl = args.outlier + D.obs_off;
    dsdtm_local_ba_summary* sm = args.summary + blockIdx.x;
    Ws w;
    ws_layout(p.NP, p.N, args.ws + D.ws_off, &w);

    // the problem passed local_ba_check_kernel (same stream, before this launch): indices, levels, order and limits hold
    // ---- 1. set-up: free slots, parameter blocks, point runs, the pair lists of the reduced camera matrix
    if (tid < p.K) sh.ired[tid] = 0;
    __syncthreads();
    for (int i = tid; i < p.N; i += NT) sh.ired[p.okf[i]] = 1;      // observed keyframes (same value from every writer)
    __syncthreads();
    if (tid == 0) {
        int nf = 0;
        for (int k = 0; k < p.K; ++k) {
            const bool fr = !p.kc[k] && sh.ired[k];
            sh.slot[k] = fr ? nf : -1;
            if (fr) sh.slot_kf[nf++] = k;
        }
        sh.nf = nf;
    }
    if (tid < p.K) {                                             // KeyFrame::Get_Pose(): [t, log R] (:172-175)
        const SE3d T0 = se3_from_rt(p.T_io + 12 * (size_t)tid);
        double* x = sh.x[tid];
        x[0] = T0.tx; x[1] = T0.ty; x[2] = T0.tz;
        so3_log<LAT>(T0, x + 3);
        set_pose(sh, tid, x);
    }
    for (int i = tid; i < p.N; i += NT) {                        // pt_start: first observation of every point
        const int q = p.opt[i];
        const int prev = i == 0 ? -1 : p.opt[i - 1];
        for (int r = prev + 1; r <= q; ++r) w.pt_start[r] = i;
        if (i == p.N - 1)
            for (int r = q + 1; r <= p.NP; ++r) w.pt_start[r] = p.N;
    }
    if (p.N == 0)
        for (int r = tid; r <= p.NP; r += NT) w.pt_start[r] = 0;
    for (size_t e = tid; e < (size_t)p.NP * MAXF; e += NT) w.table[e] = -1;
    __syncthreads();
    const int nf = sh.nf;
    const int nblk = nf * (nf + 1) / 2;
    for (int i = tid; i < p.N; i += NT) {
        const int a = sh.slot[p.okf[i]];
        if (a >= 0) w.table[(size_t)p.opt[i] * MAXF + a] = i;
    }
    __syncthreads();
    int my_a = -1, my_b = -1;
    if (tid < nblk) {
        block_ab(tid, nf, my_a, my_b);
        int cnt = 0;
        for (int q = 0; q < p.NP; ++q) {
            const int32_t* t = w.table + (size_t)q * MAXF;
            cnt += (t[my_a] >= 0 && t[my_b] >= 0) ? 1 : 0;
        }
        sh.ired[tid] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int b = 0; b < nblk; ++b) { sh.pair_off[b] = o; o += sh.ired[b]; }
        sh.pair_off[nblk] = o;
    }
    __syncthreads();
    if (tid < nblk) {
        int o = sh.pair_off[tid];
        for (int q = 0; q < p.NP; ++q) {
            const int32_t* t = w.table + (size_t)q * MAXF;
            const int i = t[my_a], j = t[my_b];
            if (i >= 0 && j >= 0) { w.pairs[2 * (size_t)o] = i; w.pairs[2 * (size_t)o + 1] = j; ++o; }
        }
    }
    __syncthreads();

    int termination = DSDTM_PO_NO_RESIDUALS, iterations = 0, successful = 0;
    double cost = 0.0, initial_cost = 0.0;
    if (p.N > 0) {
        int finite;
        cost = eval_all(sh, p, w, false, &finite);
        if (!finite) {
            termination = DSDTM_PO_EVALUATION_FAILED;
            cost = 0.0;
        } else {
            initial_cost = cost;
            // Jacobi scaling 1 / (1 + |column|), fixed at iteration 0 (points: workspace, poses: sh.kscale)
            for (int q = tid; q < p.NP; q += NT) {
                double c2[3] = {0.0, 0.0, 0.0};
                for (int i = w.pt_start[q]; i < w.pt_start[q + 1]; ++i) {
                    const double* row = w.J + (size_t)i * JS;
#pragma unroll
                    for (int c = 0; c < 3; ++c) c2[c] += row[14 + c] * row[14 + c] + row[17 + c] * row[17 + c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) w.P[(size_t)q * PS + P_SCALE + c] = 1.0 / (1.0 + sqrt(c2[c]));
            }
            {
                const int a = tid - KF_THREAD0;
                if (a >= 0 && a < nf) {
                    double c2[6] = {0, 0, 0, 0, 0, 0};
                    const int b = a * nf - a * (a - 1) / 2;
                    for (int e = sh.pair_off[b]; e < sh.pair_off[b + 1]; ++e) {
                        const double* row = w.J + (size_t)w.pairs[2 * (size_t)e] * JS;
#pragma unroll
                        for (int c = 0; c < 6; ++c) c2[c] += row[2 + c] * row[2 + c] + row[8 + c] * row[8 + c];
                    }
#pragma unroll
                    for (int c = 0; c < 6; ++c) sh.kscale[a][c] = 1.0 / (1.0 + sqrt(c2[c]));
                }
            }
            __syncthreads();
            for (int i = tid; i < p.N; i += NT) {                 // scale the stored Jacobians in place
                double* row = w.J + (size_t)i * JS;
                const int a = sh.slot[p.okf[i]];
                const double* ps = w.P + (size_t)p.opt[i] * PS + P_SCALE;
                if (a >= 0) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) { row[2 + c] *= sh.kscale[a][c]; row[8 + c] *= sh.kscale[a][c]; }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) { row[14 + c] *= ps[c]; row[17 + c] *= ps[c]; }
            }
            __syncthreads();
            double gmax = gradient(sh, p, w);
            double xnorm = x_norm(sh, p, w);
            double radius = 1e4, decrease_factor = 2.0;
            bool reuse_diagonal = false;
            int invalid_steps = 0, it = 0;
            const int n = 6 * nf;
            for (;;) {
                if (it >= args.max_iterations) { termination = DSDTM_PO_MAX_ITERATIONS; break; }
                if (gmax <= 1e-10) { termination = DSDTM_PO_GRADIENT_TOLERANCE; break; }
                if (radius <= 1e-32) { termination = DSDTM_PO_MIN_RADIUS; break; }
                ++it;
                // -- points: V' + D^2, its inverse, F_i = W'_i V^-1
                int fail = 0;
                for (int q = tid; q < p.NP; q += NT) {
                    const int i0 = w.pt_start[q], i1 = w.pt_start[q + 1];
                    if (i0 == i1) continue;
                    double V[6] = {0, 0, 0, 0, 0, 0};
                    for (int i = i0; i < i1; ++i) {
                        const double* jp = w.J + (size_t)i * JS + 14;
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = r; c < 3; ++c) V[sym3(r, c)] += jp[r] * jp[c] + jp[3 + r] * jp[3 + c];
                    }
                    double* P = w.P + (size_t)q * PS;
                    if (!reuse_diagonal) {
                        P[P_DIAG + 0] = fmin(fmax(V[0], 1e-6), 1e32);
                        P[P_DIAG + 1] = fmin(fmax(V[3], 1e-6), 1e32);
                        P[P_DIAG + 2] = fmin(fmax(V[5], 1e-6), 1e32);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double lm = sqrt(P[P_DIAG + c] / radius);
                        V[sym3(c, c)] += lm * lm;
                    }
                    // 3x3 Cholesky, then V^-1 = L^-T L^-1
                    double vi[6];
                    const double l00 = sqrt(V[0]);
                    const double l10 = V[1] / l00, l20 = V[2] / l00;
                    const double d11 = V[3] - l10 * l10;
                    const double l11 = sqrt(d11);
                    const double l21 = (V[4] - l20 * l10) / l11;
                    const double d22 = V[5] - l20 * l20 - l21 * l21;
                    const double l22 = sqrt(d22);
                    if (!(V[0] > 0.0 && d11 > 0.0 && d22 > 0.0)) {
                        fail = 1;
#pragma unroll
                        for (int k = 0; k < 6; ++k) vi[k] = __builtin_nan("");
                    } else {
                        const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
                        const double i10 = -l10 * i00 * i11;
                        const double i21 = -l21 * i11 * i22;
                        const double i20 = -(l20 * i00 + l21 * i10) * i22;
                        vi[0] = i00 * i00 + i10 * i10 + i20 * i20;
                        vi[1] = i10 * i11 + i20 * i21;
                        vi[2] = i20 * i22;
                        vi[3] = i11 * i11 + i21 * i21;
                        vi[4] = i21 * i22;
                        vi[5] = i22 * i22;
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) P[P_VINV + k] = vi[k];
                    for (int i = i0; i < i1; ++i) {
                        if (sh.slot[p.okf[i]] < 0) continue;
                        const double* row = w.J + (size_t)i * JS;
                        double* F = w.F + (size_t)i * FS;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            double W[3];
#pragma unroll
                            for (int c = 0; c < 3; ++c) W[c] = row[2 + r] * row[14 + c] + row[8 + r] * row[17 + c];
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                F[3 * r + c] = W[0] * vi[sym3(0, c)] + W[1] * vi[sym3(1, c)] + W[2] * vi[sym3(2, c)];
                        }
                    }
                }
                __syncthreads();
                // -- the reduced camera matrix: pairs (threads [0, nblk)), pose blocks (threads [KF_THREAD0, + nf))
                if (tid < nblk) {
                    double acc[36];
#pragma unroll
                    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
                    for (int e = sh.pair_off[tid]; e < sh.pair_off[tid + 1]; ++e) {
                        const int i = w.pairs[2 * (size_t)e], j = w.pairs[2 * (size_t)e + 1];
                        const double* F = w.F + (size_t)i * FS;
                        const double* rj = w.J + (size_t)j * JS;
                        double G[12];                           // F_i Jp'_j^T (6x2)
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            G[2 * r] = F[3 * r] * rj[14] + F[3 * r + 1] * rj[15] + F[3 * r + 2] * rj[16];
                            G[2 * r + 1] = F[3 * r] * rj[17] + F[3 * r + 1] * rj[18] + F[3 * r + 2] * rj[19];
                        }
#pragma unroll
                        for (int r = 0; r < 6; ++r)
#pragma unroll
                            for (int c = 0; c < 6; ++c) acc[6 * r + c] += G[2 * r] * rj[2 + c] + G[2 * r + 1] * rj[8 + c];
                    }
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            sh.S[(6 * my_a + r) * MAXN + 6 * my_b + c] = -acc[6 * r + c];
                            if (my_a != my_b) sh.S[(6 * my_b + c) * MAXN + 6 * my_a + r] = -acc[6 * r + c];
                        }
                }
                {
                    const int a = tid - KF_THREAD0;
                    if (a >= 0 && a < nf) {
                        double U[21], bp[6];
#pragma unroll
                        for (int k = 0; k < 21; ++k) U[k] = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; ++k) bp[k] = 0.0;
                        const int b = a * nf - a * (a - 1) / 2;
                        for (int e = sh.pair_off[b]; e < sh.pair_off[b + 1]; ++e) {
                            const int i = w.pairs[2 * (size_t)e];
                            const double* row = w.J + (size_t)i * JS;
                            const double* F = w.F + (size_t)i * FS;
                            const double* g = w.P + (size_t)p.opt[i] * PS + P_G;
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
#pragma unroll
                                for (int c = r; c < 6; ++c) U[sym6(r, c)] += row[2 + r] * row[2 + c] + row[8 + r] * row[8 + c];
                                bp[r] += F[3 * r] * g[0] + F[3 * r + 1] * g[1] + F[3 * r + 2] * g[2];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 21; ++k) sh.U[a][k] = U[k];
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            sh.rhs[6 * a + r] = sh.kg[a][r] - bp[r];
                            if (!reuse_diagonal) sh.kdiag[a][r] = fmin(fmax(U[sym6(r, r)], 1e-6), 1e32);
                        }
                    }
                }
                __syncthreads();
                for (int e = tid; e < 36 * nf; e += NT) {           // S_aa += U'_a + D_a^2
                    const int a = e / 36, r = (e % 36) / 6, c = e % 6;
                    double v = sh.U[a][sym6(r, c)];
                    if (r == c) { const double lm = sqrt(sh.kdiag[a][r] / radius); v += lm * lm; }
                    sh.S[(6 * a + r) * MAXN + 6 * a + c] += v;
                }
                // -- Cholesky of S (lower, in place), right-looking
                for (int k = 0; k < n; ++k) {
                    __syncthreads();
                    const double dkk = sh.S[k * MAXN + k];
                    if (!(dkk > 0.0)) { fail = 1; break; }          // uniform: every thread reads the same value
                    const double lkk = sqrt(dkk);
                    __syncthreads();
                    if (tid == 0) sh.S[k * MAXN + k] = lkk;
                    for (int i = k + 1 + tid; i < n; i += NT) sh.S[i * MAXN + k] /= lkk;
                    __syncthreads();
                    const int m = n - k - 1;
                    for (int e = tid; e < m * (m + 1) / 2; e += NT) {     // the lower triangle only: row r, column c <= r
                        int r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
                        while (r * (r + 1) / 2 > e) --r;
                        while ((r + 1) * (r + 2) / 2 <= e) ++r;
                        const int i = k + 1 + r, j = k + 1 + (e - r * (r + 1) / 2);
                        sh.S[i * MAXN + j] -= sh.S[i * MAXN + k] * sh.S[j * MAXN + k];
                    }
                }
                __syncthreads();
                fail = block_or(sh, fail);
                // -- substitutions by wave 0 (lane l holds rows l and l + 64)
                if (!fail && tid < 64) {
                    double y0 = tid < n ? sh.rhs[tid] : 0.0, y1 = tid + 64 < n ? sh.rhs[tid + 64] : 0.0;
                    for (int k = 0; k < n; ++k) {                   // L y = b
                        const double bk = __shfl(k < 64 ? y0 : y1, k & 63);
                        const double yk = bk / sh.S[k * MAXN + k];
                        if (tid == (k & 63)) { if (k < 64) y0 = yk; else y1 = yk; }
                        if (tid > k && tid < n) y0 -= sh.S[tid * MAXN + k] * yk;
                        if (tid + 64 > k && tid + 64 < n) y1 -= sh.S[(tid + 64) * MAXN + k] * yk;
                    }
                    for (int k = n - 1; k >= 0; --k) {              // L^T z = y
                        const double bk = __shfl(k < 64 ? y0 : y1, k & 63);
                        const double zk = bk / sh.S[k * MAXN + k];
                        if (tid == (k & 63)) { if (k < 64) y0 = zk; else y1 = zk; }
                        if (tid < k) y0 -= sh.S[k * MAXN + tid] * zk;
                        if (tid + 64 < k) y1 -= sh.S[k * MAXN + tid + 64] * zk;
                    }
                    if (tid < n) sh.kstep[tid / 6][tid % 6] = -y0;
                    if (tid + 64 < n) sh.kstep[(tid + 64) / 6][(tid + 64) % 6] = -y1;
                }
                __syncthreads();
                // -- back-substitution: y_p = V^-1 (g'_p - sum W'_i^T y_a); step = -y
                int nonfinite = fail;
                if (!fail) {
                    for (int q = tid; q < p.NP; q += NT) {
                        const int i0 = w.pt_start[q], i1 = w.pt_start[q + 1];
                        if (i0 == i1) continue;
                        double* P = w.P + (size_t)q * PS;
                        double t[3] = {P[P_G], P[P_G + 1], P[P_G + 2]};
                        for (int i = i0; i < i1; ++i) {
                            const int a = sh.slot[p.okf[i]];
                            if (a < 0) continue;
                            const double* row = w.J + (size_t)i * JS;
                            double u0 = 0.0, u1 = 0.0;              // Jc'_i y_a = -(Jc'_i step_a)
#pragma unroll
                            for (int c = 0; c < 6; ++c) { u0 -= row[2 + c] * sh.kstep[a][c]; u1 -= row[8 + c] * sh.kstep[a][c]; }
#pragma unroll
                            for (int c = 0; c < 3; ++c) t[c] -= row[14 + c] * u0 + row[17 + c] * u1;
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double y = P[P_VINV + sym3(c, 0)] * t[0] + P[P_VINV + sym3(c, 1)] * t[1] + P[P_VINV + sym3(c, 2)] * t[2];
                            P[P_STEP + c] = -y;
                            nonfinite |= isfinite(y) ? 0 : 1;
                        }
                    }
                    if (tid < n) nonfinite |= isfinite(sh.kstep[tid / 6][tid % 6]) ? 0 : 1;
                }
                __syncthreads();
                nonfinite = block_or(sh, nonfinite);
                // -- model decrease from J * step: -(J s) . (r + J s / 2)
                double model_cost_change = 0.0;
                if (!nonfinite) {
                    double part = 0.0;
                    for (int i = tid; i < p.N; i += NT) {
                        const double* row = w.J + (size_t)i * JS;
                        const double* st = w.P + (size_t)p.opt[i] * PS + P_STEP;
                        const int a = sh.slot[p.okf[i]];
                        double m0 = row[14] * st[0] + row[15] * st[1] + row[16] * st[2];
                        double m1 = row[17] * st[0] + row[18] * st[1] + row[19] * st[2];
                        if (a >= 0) {
                            double c0 = 0.0, c1 = 0.0;
#pragma unroll
                            for (int c = 0; c < 6; ++c) { c0 += row[2 + c] * sh.kstep[a][c]; c1 += row[8 + c] * sh.kstep[a][c]; }
                            m0 = c0 + m0; m1 = c1 + m1;
                        }
                        part += m0 * (row[0] + m0 / 2.0) + m1 * (row[1] + m1 / 2.0);
                    }
                    model_cost_change = -block_sum(sh, part);
                }
                reuse_diagonal = true;
                if (nonfinite || !(model_cost_change > 0.0)) {
                    if (++invalid_steps >= 5) { termination = DSDTM_PO_INVALID_STEPS; break; }
                    radius = radius / decrease_factor;
                    decrease_factor *= 2.0;
                    continue;
                }
                invalid_steps = 0;
                // -- candidate: Plus for the poses, vector sum for the points; |x - x_cand|
                double dn = 0.0;
                if (tid < nf) {
                    double d[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c) d[c] = sh.kstep[tid][c] * sh.kscale[tid][c];
                    const double* x = sh.x[sh.slot_kf[tid]];
                    pose_plus<LAT>(pose_of<LAT>(x), d, sh.xc[tid]);
                    const SE3d Tc = pose_of<LAT>(sh.xc[tid]);
                    sh.Tc[tid][0] = Tc.qw; sh.Tc[tid][1] = Tc.qx; sh.Tc[tid][2] = Tc.qy; sh.Tc[tid][3] = Tc.qz;
                    sh.Tc[tid][4] = Tc.tx; sh.Tc[tid][5] = Tc.ty; sh.Tc[tid][6] = Tc.tz;
#pragma unroll
                    for (int c = 0; c < 6; ++c) { const double v = x[c] - sh.xc[tid][c]; dn += v * v; }
                }
                for (int q = tid; q < p.NP; q += NT) {
                    if (w.pt_start[q] == w.pt_start[q + 1]) continue;
                    double* P = w.P + (size_t)q * PS;
                    const double* X = p.X + 3 * (size_t)q;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        P[P_CAND + c] = X[c] + P[P_STEP + c] * P[P_SCALE + c];
                        const double v = X[c] - P[P_CAND + c];
                        dn += v * v;
                    }
                }
                __syncthreads();
                const double step_norm = sqrt(block_sum(sh, dn));
                // -- cost at the candidate
                double part = 0.0;
                for (int i = tid; i < p.N; i += NT) {
                    const int k = p.okf[i], a = sh.slot[k];
                    part += eval_obs<false>(p, i, a >= 0 ? sh.Tc[a] : sh.T[k], nullptr, w.P + (size_t)p.opt[i] * PS + P_CAND, nullptr);
                }
                double cand_cost = block_sum(sh, part);
                if (!isfinite(cand_cost)) cand_cost = DBL_MAX;
                if (step_norm <= 1e-8 * (xnorm + 1e-8)) { termination = DSDTM_PO_PARAMETER_TOLERANCE; break; }
                const double cost_change = cost - cand_cost;
                if (fabs(cost_change) <= 1e-6 * cost) { termination = DSDTM_PO_FUNCTION_TOLERANCE; break; }
                const double relative_decrease = cost_change / model_cost_change;
                if (relative_decrease > 1e-3) {
                    if (tid < nf) {
                        const int k = sh.slot_kf[tid];
#pragma unroll
                        for (int c = 0; c < 6; ++c) sh.x[k][c] = sh.xc[tid][c];
                        set_pose(sh, k, sh.x[k]);
                    }
                    for (int q = tid; q < p.NP; q += NT) {
                        if (w.pt_start[q] == w.pt_start[q + 1]) continue;
                        const double* P = w.P + (size_t)q * PS;
#pragma unroll
                        for (int c = 0; c < 3; ++c) p.X[3 * (size_t)q + c] = P[P_CAND + c];
                    }
                    __syncthreads();
                    int finite2;
                    cost = eval_all(sh, p, w, true, &finite2);
                    ++successful;
                    // Ceres ends the solve when the Jacobian evaluation at the accepted point fails (its cost was finite)
                    if (!finite2) { termination = DSDTM_PO_EVALUATION_FAILED; break; }
                    gmax = gradient(sh, p, w);
                    xnorm = x_norm(sh, p, w);
                    const double t = 2.0 * relative_decrease - 1.0;
                    radius = radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
                    radius = fmin(1e16, radius);
                    decrease_factor = 2.0;
                    reuse_diagonal = false;
                } else {
                    radius = radius / decrease_factor;
                    decrease_factor *= 2.0;
                    reuse_diagonal = true;
                }
            }
            iterations = it;
        }
    }
    __syncthreads();

    // ---- write-back (:236-248): every keyframe SE3(SO3::exp(x.tail), x.head); the points were updated in place
    if (tid < p.K) {
        double* To = p.T_io + 12 * (size_t)tid;
        const double* R = sh.R[tid];
        const double* q = sh.T[tid];
        To[0] = R[0]; To[1] = R[1]; To[2] = R[2];  To[3] = q[4];
        To[4] = R[3]; To[5] = R[4]; To[6] = R[5];  To[7] = q[5];
        To[8] = R[6]; To[9] = R[7]; To[10] = R[8]; To[11] = q[6];
    }
    // ---- outlier pass (:250-271): utils::ReprojectionError at the new poses against delta^2
    const double thr = p.delta * p.delta;
    int n_out = 0;
    for (int i = tid; i < p.N; i += NT) {
        const int k = p.okf[i];
        SE3d T;
        T.qw = sh.T[k][0]; T.qx = sh.T[k][1]; T.qy = sh.T[k][2]; T.qz = sh.T[k][3];
        T.tx = sh.T[k][4]; T.ty = sh.T[k][5]; T.tz = sh.T[k][6];
        const double* X = p.X + 3 * (size_t)p.opt[i];
        double rx, ry, rz;
        quat_rotate(T, X[0], X[1], X[2], rx, ry, rz);
        const double px = rx + T.tx, py = ry + T.ty, pz = rz + T.tz;
        const double b0 = p.bear[3 * (size_t)i], b1 = p.bear[3 * (size_t)i + 1], b2 = p.bear[3 * (size_t)i + 2];
        const double e0 = b0 / b2 - px / pz, e1 = b1 / b2 - py / pz;
        const uint8_t o = (e0 * e0 + e1 * e1) > thr ? 1 : 0;
        p.outl[i] = o;
        n_out += o;
    }
    sh.ired[tid] = n_out;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int k = 0; k < NT; ++k) s += sh.ired[k];
        dsdtm_local_ba_summary out = {};
        out.iterations = iterations;
        out.successful_steps = successful;
        out.termination = termination;
        out.n_residual_blocks = p.N;
        out.n_outliers = s;
        out.n_free_keyframes = sh.nf;
        out.initial_cost = initial_cost;
        out.final_cost = cost;
        *sm = out;
    }
}

// The checks the host cannot make on device arrays, one workgroup per problem: writes a.check[problem] = a mask of
// LBA_CHECK_* (0: the problem is valid). Reads only; the entry point reads the masks back before it enqueues the solve.
__global__ __launch_bounds__(NT) void local_ba_check_kernel(LocalBaArgs a) {
    __shared__ int ired[NT];
    const int tid = threadIdx.x;
    const LocalBaProblemDev D = a.problems[blockIdx.x];
    const int K = D.n_kf, NP = D.n_pts, N = D.n_obs;
    const uint8_t* kc = a.kf_const + D.kf_off;
    const int32_t* okf = a.obs_kf + D.obs_off;
    const int32_t* opt = a.obs_pt + D.obs_off;
    const int32_t* lev = a.level + D.obs_off;
    int bad = 0;
    for (int i = tid; i < N; i += NT) {
        const int k = okf[i], q = opt[i], l = lev[i];
        if (k < 0 || k >= K) bad |= LBA_CHECK_KF_INDEX;
        if (q < 0 || q >= NP) bad |= LBA_CHECK_POINT_INDEX;
        if (l < 0 || l >= DSDTM_MAX_LEVELS) bad |= LBA_CHECK_LEVEL;
        if (i > 0 && opt[i - 1] > q) bad |= LBA_CHECK_ORDER;
        if (q >= 0 && !(bad & LBA_CHECK_ORDER))
            for (int j = i - 1; j >= 0 && opt[j] == q; --j)      // a run holds <= K distinct keyframes when it is valid
                if (okf[j] == k) { bad |= LBA_CHECK_DUPLICATE; break; }
    }
    if (tid == 0) {
        int nfree = 0;
        for (int k = 0; k < K; ++k) nfree += kc[k] ? 0 : 1;
        if (nfree == 0) bad |= LBA_CHECK_NO_FREE;
        if (nfree > MAXF) bad |= LBA_CHECK_FREE_LIMIT;
        if (K - nfree > DSDTM_LBA_MAX_CONST_KF) bad |= LBA_CHECK_CONST_LIMIT;
    }
    ired[tid] = bad;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) ired[tid] |= ired[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.check[blockIdx.x] = ired[0];
}

__global__ __launch_bounds__(NT) void local_ba_kernel(LocalBaArgs a) {
    __shared__ Shared sh;
    local_ba_body(a, sh);
}

}  // namespace

size_t local_ba_workspace_bytes(int n_pts, int n_obs) { return ws_layout(n_pts, n_obs, nullptr, nullptr); }

hipError_t local_ba_check_launch(const LocalBaArgs& args, hipStream_t stream) {
    if (args.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(local_ba_check_kernel, dim3((unsigned)args.n_problems), dim3(NT), 0, stream, args);
    return hipGetLastError();
}

hipError_t local_ba_launch(const LocalBaArgs& args, hipStream_t stream) {
    if (args.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(local_ba_kernel, dim3((unsigned)args.n_problems), dim3(NT), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
