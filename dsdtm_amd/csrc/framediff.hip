// framediff.hip — the kernels of libdsdtm_amd_framediff.so (include/dsdtm_amd_framediff.h), gfx950, 64-lane wavefronts.
//
//   framediff_kernel            F2-F7 for n pairs in ONE launch: blockIdx.y is the pair, blockIdx.x a band of R = FRAMEDIFF_ROWS output rows
//                               at full width. The workgroup (16 wavefronts) evaluates F2-F5 for R + 12 rows (6 halo rows either side,
//                               2 per pass of F6): a wavefront takes 64 consecutive pixels of a row — the map in double, every multiply
//                               and add rounded on its own (no contraction: see dm / da), the four taps of b, the byte of a — and __ballot
//                               turns the 64 comparisons into the row's word of a bit-plane in LDS: t never exists as bytes. The
//                               three passes of F6 work on words: a horizontal pass is two shifts either way with the carry of the
//                               neighbouring word, a vertical pass the AND / OR of five row words; two planes of (R + 12) x
//                               ceil(W / 64) words take turns. A word is read through plane_word(), which answers the pass's neutral
//                               value (1 for the AND, 0 for the ORs) for a row above row 0 or below the last row, for a word left or
//                               right of the image and for the bits of the last word beyond the width — at EVERY pass, so an e or o
//                               value at an outside position never feeds the next one. The R rows leave as 32-bit stores of four mask
//                               bytes (bytes where the address or the tail forbids it); n_foreground is __popcll over the band's
//                               words, one LDS atomic per wavefront and ONE integer global atomic per workgroup (an integer sum: its
//                               order is free). Lanes beyond the width and rows beyond the image read no pixel.
//   framediff_features_kernel   F8: one thread per feature against the mask where it lies (motion.hip's test).
//   framediff_warp_kernel       F2-F3 alone: one thread per destination pixel.
// No kernel waits for another workgroup. Plain HIP C++ only.
#include "framediff.h"

namespace dsdtm {

typedef unsigned long long word_t;

// F2 rounds every product and sum on its own: plain `*` and `+` under a FILE-scope pragma. Not __dmul_rn / __dadd_rn: they are inline
// functions of the HIP headers, compiled under the headers' setting (contraction allowed), and once inlined M0*x + M1*y came out as a
// fused multiply-add whatever pragma stood in the caller — which showed on the device as cvRound ties going the other way.
#pragma clang fp contract(off)

__device__ __forceinline__ double dm(double a, double b) { return a * b; }
__device__ __forceinline__ double da(double a, double b) { return a + b; }

// F2's end: NaN is "outside"; otherwise clamped to int32, then cvRound (halves to even: the default rounding mode)
__device__ __forceinline__ int32_t map_round(double v) {
    if (v != v) return -2147483647 - 1;
    v = fmin(fmax(v, -2147483648.0), 2147483647.0);
    return (int32_t)rint(v);
}

__device__ __forceinline__ uint32_t b_tap(const uint8_t* __restrict__ src, int stride, int w, int h, int x, int y) {
    return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? (uint32_t)src[(size_t)y * (size_t)stride + (size_t)x] : 0u;
}

// F2 + F3 for the destination pixel (x, y)
__device__ __forceinline__ uint32_t warp_sample(const FrameDiffDev& r, int x, int y) {
    const double xd = (double)x, yd = (double)y;
    const double X0 = da(da(dm(r.M[0], xd), dm(r.M[1], yd)), r.M[2]);
    const double Y0 = da(da(dm(r.M[3], xd), dm(r.M[4], yd)), r.M[5]);
    const double W = da(da(dm(r.M[6], xd), dm(r.M[7], yd)), r.M[8]);
    const double s = W != 0.0 ? 32.0 / W : 0.0;
    const int32_t X = map_round(dm(X0, s)), Y = map_round(dm(Y0, s));
    const int x0 = X >> 5, ax = X & 31, y0 = Y >> 5, ay = Y & 31;
    const uint32_t p00 = b_tap(r.b, r.b_stride, r.w, r.h, x0, y0), p01 = b_tap(r.b, r.b_stride, r.w, r.h, x0 + 1, y0);
    const uint32_t p10 = b_tap(r.b, r.b_stride, r.w, r.h, x0, y0 + 1), p11 = b_tap(r.b, r.b_stride, r.w, r.h, x0 + 1, y0 + 1);
    return ((uint32_t)((32 - ax) * (32 - ay)) * p00 + (uint32_t)(ax * (32 - ay)) * p01 + (uint32_t)((32 - ax) * ay) * p10 + (uint32_t)(ax * ay) * p11 + 512u) >> 10;
}

// The word k of plane row rr (image row y) as a pass of F6 reads it: `fill` (all ones for the AND, zero for the ORs) for everything
// outside the image — a row, a word, the bits of the last word beyond the width
__device__ __forceinline__ word_t plane_word(const word_t* plane, int nw, int rr, int k, int y, int h, word_t last_valid, word_t fill) {
    if (y < 0 || y >= h || k < 0 || k >= nw) return fill;
    const word_t v = plane[rr * nw + k];
    return k == nw - 1 ? (v & last_valid) | (fill & ~last_valid) : v;
}

// one pass of F6 over the plane rows [lo, hi): dst = AND / OR of src over the 5x5 window (bit i of word k is pixel 64 k + i)
template <bool IS_AND>
__device__ __forceinline__ void morph_pass(const word_t* src, word_t* dst, int nw, int lo, int hi, int y_first, int h, word_t last_valid) {
    const word_t fill = IS_AND ? ~(word_t)0 : (word_t)0;
    for (int item = (int)threadIdx.x; item < (hi - lo) * nw; item += FRAMEDIFF_THREADS) {
        const int rr = lo + item / nw, k = item % nw, y = y_first + rr;
        if (y < 0 || y >= h) continue;      // dst keeps stale words in such a row. INVARIANT: every reader of a plane goes through plane_word(), which answers for it
        word_t acc = fill;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const word_t c = plane_word(src, nw, rr + dy, k, y + dy, h, last_valid, fill);
            const word_t p = plane_word(src, nw, rr + dy, k - 1, y + dy, h, last_valid, fill);
            const word_t n = plane_word(src, nw, rr + dy, k + 1, y + dy, h, last_valid, fill);
            const word_t l1 = (c << 1) | (p >> 63), l2 = (c << 2) | (p >> 62), r1 = (c >> 1) | (n << 63), r2 = (c >> 2) | (n << 62);
            acc = IS_AND ? (acc & c & l1 & l2 & r1 & r2) : (acc | c | l1 | l2 | r1 | r2);
        }
        dst[rr * nw + k] = acc;
    }
}

__global__ __launch_bounds__(FRAMEDIFF_THREADS) void framediff_kernel(const FrameDiffDev* __restrict__ recs, int max_nw) {
    extern __shared__ word_t planes[];
    __shared__ int band_count;
    const FrameDiffDev& r = recs[blockIdx.y];                // (uniform)
    constexpr int R = FRAMEDIFF_ROWS, ROWS = R + 2 * FRAMEDIFF_HALO;
    const int y0 = (int)blockIdx.x * R;
    if (y0 >= r.h) return;                                   // (the whole workgroup)
    const int w = r.w, h = r.h, nw = (w + 63) >> 6, y_first = y0 - FRAMEDIFF_HALO;
    const word_t last_valid = (w & 63) ? (((word_t)1 << (w & 63)) - 1) : ~(word_t)0;
    word_t* A = planes;
    word_t* B = planes + ROWS * max_nw;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (threadIdx.x == 0) band_count = 0;
    // F2-F5: t, one word per wavefront and step
    for (int item = wave; item < ROWS * nw; item += FRAMEDIFF_THREADS / 64) {
        const int rr = item / nw, k = item - rr * nw, y = y_first + rr, x = 64 * k + lane;
        if (y < 0 || y >= h) continue;                       // (the wavefront as one)
        bool on = false;
        if (x < w) {
            const uint32_t wv = warp_sample(r, x, y);
            if (r.warped && rr >= FRAMEDIFF_HALO && rr < FRAMEDIFF_HALO + R) r.warped[(size_t)y * (size_t)r.warped_stride + (size_t)x] = (uint8_t)wv;
            const int d = (int)r.a[(size_t)y * (size_t)r.a_stride + (size_t)x] - (int)wv;          // F4: max(d, 0) > threshold is d > threshold
            on = d > r.threshold;
        }
        const word_t bits = __ballot(on);
        if (lane == 0) A[item] = bits;
    }
    __syncthreads();
    morph_pass<true>(A, B, nw, 2, ROWS - 2, y_first, h, last_valid);           // e
    __syncthreads();
    morph_pass<false>(B, A, nw, 4, ROWS - 4, y_first, h, last_valid);          // o
    __syncthreads();
    morph_pass<false>(A, B, nw, 6, ROWS - 6, y_first, h, last_valid);          // f
    __syncthreads();
    // F7 and the counter of F8
    const int rows = min(R, h - y0);
    int count = 0;
    for (int item = (int)threadIdx.x; item < rows * nw; item += FRAMEDIFF_THREADS) {
        const int j = item / nw, k = item - j * nw;
        word_t v = B[(FRAMEDIFF_HALO + j) * nw + k];
        if (k == nw - 1) v &= last_valid;
        count += __popcll(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (lane == 0 && count) atomicAdd(&band_count, count);
    if (r.mask) {
        const int nq = (w + 3) >> 2;
        const uint32_t mv = (uint32_t)r.maxval;
        for (int item = (int)threadIdx.x; item < rows * nq; item += FRAMEDIFF_THREADS) {
            const int j = item / nq, q = item - j * nq, x = 4 * q;
            const uint32_t bits = (uint32_t)(B[(FRAMEDIFF_HALO + j) * nw + (x >> 6)] >> (x & 63)) & 0xFu;
            uint8_t* p = r.mask + (size_t)(y0 + j) * (size_t)r.mask_stride + (size_t)x;
            if (x + 4 <= w && ((uintptr_t)p & 3) == 0) {
                *reinterpret_cast<uint32_t*>(p) = ((bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21)) * mv;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (x + i < w) p[i] = (bits >> i) & 1u ? (uint8_t)mv : (uint8_t)0;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && band_count) atomicAdd(r.n_foreground, band_count);
}

// Frame::Motion_Removal's test (src/Frame.cpp:352) against the mask where it lies: cvRound rounds halves to even (rintf)
__global__ __launch_bounds__(256) void framediff_features_kernel(const FrameDiffDev* __restrict__ recs) {
    const FrameDiffDev& r = recs[blockIdx.y];
    const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (f >= r.n_feat) return;
    const float fx = rintf(r.feat[2 * (size_t)f]), fy = rintf(r.feat[2 * (size_t)f + 1]);
    uint8_t on = 0;
    if (fx >= 0.0f && fx < (float)r.w && fy >= 0.0f && fy < (float)r.h)        // (the host refused anything else)
        on = r.mask[(size_t)(int)fy * (size_t)r.mask_stride + (size_t)(int)fx] == 255 ? 1 : 0;
    r.flags[f] = on;
}

__global__ __launch_bounds__(256) void framediff_warp_kernel(const FrameDiffDev* __restrict__ recs) {
    const FrameDiffDev& r = recs[blockIdx.z];
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= r.w || y >= r.h) return;
    r.warped[(size_t)y * (size_t)r.warped_stride + (size_t)x] = (uint8_t)warp_sample(r, x, y);
}

hipError_t framediff_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream) {
    if (!recs || n <= 0 || n > DSDTM_FRAMEDIFF_MAX_STEPS || max_w <= 0 || max_w > DSDTM_FRAMEDIFF_MAX_SIDE || max_h <= 0 || max_h > DSDTM_FRAMEDIFF_MAX_SIDE)
        return hipErrorInvalidValue;
    const int max_nw = (max_w + 63) / 64;
    const size_t lds = (size_t)2 * (FRAMEDIFF_ROWS + 2 * FRAMEDIFF_HALO) * (size_t)max_nw * sizeof(word_t);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((max_h + FRAMEDIFF_ROWS - 1) / FRAMEDIFF_ROWS), (unsigned)n, 1);
    hipLaunchKernelGGL(framediff_kernel, grid, dim3(FRAMEDIFF_THREADS), lds, stream, recs, max_nw);
    return hipGetLastError();
}

hipError_t framediff_features_launch(const FrameDiffDev* recs, int n, int max_features, hipStream_t stream) {
    if (!recs || n <= 0 || max_features <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(framediff_features_kernel, dim3((unsigned)((max_features + 255) / 256), (unsigned)n), dim3(256), 0, stream, recs);
    return hipGetLastError();
}

hipError_t framediff_warp_launch(const FrameDiffDev* recs, int n, int max_w, int max_h, hipStream_t stream) {
    if (!recs || n <= 0 || n > DSDTM_FRAMEDIFF_MAX_STEPS || max_w <= 0 || max_h <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(framediff_warp_kernel, dim3((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)n), dim3(64, 4, 1), 0, stream, recs);
    return hipGetLastError();
}

}  // namespace dsdtm
