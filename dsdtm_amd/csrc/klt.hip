// klt.hip — the pyramidal Lucas-Kanade of KLTWrapper::RunTrack (Thirdparty/fastMCD/src/KLTWrapper.cpp:112-148) and of
// cv::calcOpticalFlowPyrLK (Test/test_Optimizer.cpp:91): rules K2-K7 of include/dsdtm_amd_klt.h, and the two small kernels beside it
// (level 0 into a pyramid, the survivors into a homography record).
//
// klt_kernel: ONE WAVEFRONT PER POINT, four points per 256-thread workgroup. The window's pixels are spread over the 64 lanes in passes
// (100 pixels: two, 441: seven). Per level a lane samples the previous image's window value and both Scharr gradients of its pixels
// once and keeps them in registers; an iteration samples the current level, forms the two products per pixel and reduces them across the
// wavefront. All window sums are integers (a lane's partial fits 32 bits, the totals go through a 64-bit xor butterfly of two 32-bit
// shuffles), so the tree is free and EVERY lane ends up with the same totals: each lane then runs the scalar double tail itself, which
// costs nothing against one lane doing it and broadcasting, and keeps the control flow uniform without a read-first-lane. No LDS, no
// atomics, no barrier, no waiting across workgroups; the waves of a workgroup never talk to each other.
//
// Arithmetic of the tail: + - * / sqrt floor in IEEE double, no contraction (the pragma below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "klt.h"

#pragma clang fp contract(off)

namespace dsdtm {
namespace {

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, o, 64);
        const int hi = __shfl_xor((int)((unsigned long long)v >> 32), o, 64);
        v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}

struct Weights { int w00, w01, w10, w11; };

__device__ __forceinline__ Weights weights(double fx, double fy) {      // K3
    Weights w;
    w.w00 = (int)floor((1.0 - fx) * (1.0 - fy) * 16384.0 + 0.5);
    w.w01 = (int)floor(fx * (1.0 - fy) * 16384.0 + 0.5);
    w.w10 = (int)floor((1.0 - fx) * fy * 16384.0 + 0.5);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// the window value (5 fractional bits) at tap (x, y)
__device__ __forceinline__ int sample(const uint8_t* __restrict__ L, int stride, int x, int y, const Weights& w) {
    const uint8_t* __restrict__ p = L + (size_t)y * (size_t)stride + x;
    const int s = (int)p[0] * w.w00 + (int)p[1] * w.w01 + (int)p[stride] * w.w10 + (int)p[stride + 1] * w.w11;
    return (s + 256) >> 9;
}

__device__ __forceinline__ bool inside(int ix, int iy, int n, int w, int h, int ring) {     // K4
    return ix - ring >= 0 && iy - ring >= 0 && ix + n + ring <= w - 1 && iy + n + ring <= h - 1;
}

__global__ __launch_bounds__(64 * KLT_WAVES) void klt_kernel(const KltDev* __restrict__ recs) {
    const KltDev& r = recs[blockIdx.y];
    const int lane = (int)(threadIdx.x & 63u);
    const int k = (int)blockIdx.x * KLT_WAVES + (int)(threadIdx.x >> 6);
    if (k >= r.n_points) return;                       // (whole waves leave: k is uniform in a wave)
    const int win = r.window, area = win * win, levels = r.levels, max_iter = r.max_iter;
    const double half = (double)(win - 1) * 0.5, eps2 = r.eps2, min_eig = r.min_eig;
    const double ptx = (double)r.points[2 * k], pty = (double)r.points[2 * k + 1];
    const float* __restrict__ g = r.guesses ? r.guesses : r.points;
    const double top = (double)(1 << (levels - 1));
    double nx = (double)g[2 * k] / top, ny = (double)g[2 * k + 1] / top;
    int xo[KLT_MAX_PASSES], yo[KLT_MAX_PASSES];
#pragma unroll
    for (int p = 0; p < KLT_MAX_PASSES; ++p) {
        const int i = p * 64 + lane;
        yo[p] = i / win; xo[p] = i - yo[p] * win;
    }
    int used = 0, st = 1;
    double res = 0.0;
    for (int l = levels - 1; l >= 0; --l) {
        const int w = r.w[l], h = r.h[l], stride = r.stride[l];
        const uint8_t* __restrict__ I = r.prev + r.off[l];
        const uint8_t* __restrict__ J = r.cur + r.off[l];
        const double s = (double)(1 << l);
        const double pxx = ptx / s - half, pyy = pty / s - half;
        const double fpx = floor(pxx), fpy = floor(pyy);
        // (a guess may be anywhere; a point was checked by the host to be finite, and a double beyond int's range fails `inside` below
        //  through the clamp)
        const int ix = (int)fmin(fmax(fpx, -1.0e6), 1.0e6), iy = (int)fmin(fmax(fpy, -1.0e6), 1.0e6);
        if (l < levels - 1) { nx = nx * 2.0; ny = ny * 2.0; }
        if (!inside(ix, iy, win, w, h, 1)) { if (l == 0) st = 0; continue; }
        const Weights wt = weights(pxx - fpx, pyy - fpy);
        int Iw[KLT_MAX_PASSES], dx[KLT_MAX_PASSES], dy[KLT_MAX_PASSES];
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int p = 0; p < KLT_MAX_PASSES; ++p) {
            Iw[p] = dx[p] = dy[p] = 0;
            if (p * 64 + lane < area) {
                // the 4 x 4 patch around the tap: rows y - 1 .. y + 2, columns x - 1 .. x + 2 (inside the level: K4 counted the ring)
                const uint8_t* __restrict__ q = I + (size_t)(iy + yo[p] - 1) * (size_t)stride + (ix + xo[p] - 1);
                int v[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) v[a][b] = (int)q[(size_t)a * (size_t)stride + b];
                int gx[2][2], gy[2][2];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {       // K2 at (x + b, y + a): centre v[a + 1][b + 1]
                        gx[a][b] = 3 * (v[a][b + 2] - v[a][b]) + 10 * (v[a + 1][b + 2] - v[a + 1][b]) + 3 * (v[a + 2][b + 2] - v[a + 2][b]);
                        gy[a][b] = 3 * (v[a + 2][b] - v[a][b]) + 10 * (v[a + 2][b + 1] - v[a][b + 1]) + 3 * (v[a + 2][b + 2] - v[a][b + 2]);
                    }
                Iw[p] = (v[1][1] * wt.w00 + v[1][2] * wt.w01 + v[2][1] * wt.w10 + v[2][2] * wt.w11 + 256) >> 9;
                dx[p] = (gx[0][0] * wt.w00 + gx[0][1] * wt.w01 + gx[1][0] * wt.w10 + gx[1][1] * wt.w11 + 8192) >> 14;
                dy[p] = (gy[0][0] * wt.w00 + gy[0][1] * wt.w01 + gy[1][0] * wt.w10 + gy[1][1] * wt.w11 + 8192) >> 14;
                s11 += dx[p] * dx[p]; s12 += dx[p] * dy[p]; s22 += dy[p] * dy[p];
            }
        }
        // K5
        const double a11 = (double)wave_sum((long long)s11) * 9.5367431640625e-07;       // 2^-20
        const double a12 = (double)wave_sum((long long)s12) * 9.5367431640625e-07;
        const double a22 = (double)wave_sum((long long)s22) * 9.5367431640625e-07;
        const double det = a11 * a22 - a12 * a12;
        const double min_e = (a22 + a11 - sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / (2.0 * (double)area);
        if (min_e < min_eig || det < 1.1920928955078125e-07) { if (l == 0) st = 0; continue; }
        const double inv = 1.0 / det;
        double qx = nx - half, qy = ny - half, pdx = 0.0, pdy = 0.0;
        for (int j = 0; j < max_iter; ++j) {           // K6
            const double fqx = floor(qx), fqy = floor(qy);
            const int jx = (int)fmin(fmax(fqx, -1.0e6), 1.0e6), jy = (int)fmin(fmax(fqy, -1.0e6), 1.0e6);
            if (!inside(jx, jy, win, w, h, 0)) { if (l == 0) st = 0; break; }
            const Weights wj = weights(qx - fqx, qy - fqy);
            int t1 = 0, t2 = 0;
#pragma unroll
            for (int p = 0; p < KLT_MAX_PASSES; ++p)
                if (p * 64 + lane < area) {
                    const int d = sample(J, stride, jx + xo[p], jy + yo[p], wj) - Iw[p];
                    t1 += d * dx[p]; t2 += d * dy[p];
                }
            const double b1 = (double)wave_sum((long long)t1) * 9.5367431640625e-07;
            const double b2 = (double)wave_sum((long long)t2) * 9.5367431640625e-07;
            const double ddx = (a12 * b2 - a22 * b1) * inv, ddy = (a12 * b1 - a11 * b2) * inv;
            qx = qx + ddx; qy = qy + ddy;
            ++used;
            if (ddx * ddx + ddy * ddy <= eps2) break;
            if (j > 0 && fabs(ddx + pdx) < 0.01 && fabs(ddy + pdy) < 0.01) { qx = qx - ddx * 0.5; qy = qy - ddy * 0.5; break; }
            pdx = ddx; pdy = ddy;
        }
        nx = qx + half; ny = qy + half;
        if (l == 0 && st == 1) {                       // K7
            const double fqx = floor(qx), fqy = floor(qy);
            const int jx = (int)fmin(fmax(fqx, -1.0e6), 1.0e6), jy = (int)fmin(fmax(fqy, -1.0e6), 1.0e6);
            if (!inside(jx, jy, win, w, h, 0)) st = 0;
            else {
                const Weights wj = weights(qx - fqx, qy - fqy);
                int t = 0;
#pragma unroll
                for (int p = 0; p < KLT_MAX_PASSES; ++p)
                    if (p * 64 + lane < area) {
                        const int d = sample(J, stride, jx + xo[p], jy + yo[p], wj) - Iw[p];
                        t += d < 0 ? -d : d;
                    }
                res = (double)wave_sum((long long)t) / (32.0 * (double)area);
            }
        }
    }
    if (lane == 0) {
        r.out_points[2 * k] = (float)nx; r.out_points[2 * k + 1] = (float)ny;
        r.status[k] = (uint8_t)st;
        r.iterations[k] = used;
        if (r.residual) r.residual[k] = st ? (float)res : 0.0f;
    }
}

// thread = 4 pixels of a row; block y = image
__global__ __launch_bounds__(256) void klt_ingest_kernel(const KltIngest* __restrict__ recs, int quads_per_row) {
    const KltIngest& r = recs[blockIdx.y];
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const int y = (int)(i / (unsigned)quads_per_row), x = (int)(i % (unsigned)quads_per_row) * 4;
    if (y >= r.height || x >= r.width) return;
    const uint8_t* __restrict__ s = r.src + (size_t)y * (size_t)r.sstride + x;
    uint8_t* __restrict__ d = r.dst + (size_t)y * (size_t)r.dstride + x;
    const int n = r.width - x < 4 ? r.width - x : 4;
    for (int b = 0; b < n; ++b) d[b] = s[b];
}

// one wavefront per model: ordered compaction by ballot and prefix count
__global__ __launch_bounds__(64) void klt_compact_kernel(const KltCompact* __restrict__ recs) {
    const KltCompact& r = recs[blockIdx.x];
    const int lane = (int)threadIdx.x;
    int base = 0;
    for (int k0 = 0; k0 < r.n_points; k0 += 64) {
        const int k = k0 + lane;
        const bool keep = k < r.n_points && r.status[k] != 0;
        const unsigned long long b = __ballot(keep);
        if (keep) {
            const int at = base + __popcll(b & ((1ull << lane) - 1ull));
            r.a[2 * at] = r.points[2 * k]; r.a[2 * at + 1] = r.points[2 * k + 1];
            r.b[2 * at] = r.prev_points[2 * k]; r.b[2 * at + 1] = r.prev_points[2 * k + 1];
        }
        base += __popcll(b);
    }
    if (lane == 0) {
        *r.n_tracked = base;
        r.rec->m = base >= r.min_tracked ? base : 0;
    }
}

}  // namespace

hipError_t klt_ingest_launch(const KltIngest* recs, int n, int max_width, int max_height, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int quads = (max_width + 3) / 4;
    const long long threads = (long long)quads * max_height;
    hipLaunchKernelGGL(klt_ingest_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)n), dim3(256), 0, stream, recs, quads);
    return hipGetLastError();
}

hipError_t klt_launch(const KltDev* recs, int n, int max_points, hipStream_t stream) {
    if (n <= 0 || max_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(klt_kernel, dim3((unsigned)((max_points + KLT_WAVES - 1) / KLT_WAVES), (unsigned)n), dim3(64 * KLT_WAVES), 0, stream, recs);
    return hipGetLastError();
}

hipError_t klt_compact_launch(const KltCompact* recs, int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(klt_compact_kernel, dim3((unsigned)n), dim3(64), 0, stream, recs);
    return hipGetLastError();
}

}  // namespace dsdtm
