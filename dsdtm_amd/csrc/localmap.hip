// localmap.hip — Tracking::GetCloseKeyFrames (reference src/Tracking.cpp:315-345) and the keyframe and point selection of
// Tracking::UpdateLocalMap (:258-297) on a map that is resident on the device, for n descs per call (include/dsdtm_amd_localmap.h,
// rules L1-L4).
//
//   localmap_visible_kernel   one wavefront per (desc, keyframe), four per workgroup. Lanes stride the keyframe's slots 64 at a
//       time: a coalesced load of the slots, a gather of each point's 32-byte record, the test of L1, a ballot; the wavefront
//       stops at the first chunk with a hit (the reference's break — the result is an "any", so the chunk order does not matter).
//       The keyframe's answer is ONE 64-bit key: the bit pattern of its distance (L2; non-negative, so the integer order is the
//       numeric order), or all ones when it is not close.
//   localmap_select_kernel    one 256-thread workgroup per desc. n_local rounds of a workgroup argmin over (key, index) pairs,
//       integer comparisons only: ascending distance, ties in map index order (L3). Then the walk of L4 over the chosen keyframes,
//       256 slots at a time: a point is emitted when it is not bad, not in the seen-bitmap (LDS, one bit per map point) and no
//       EARLIER entry of the same chunk holds it — the first occurrence in walk order wins whatever the timing; positions come
//       from a prefix sum over the emit flags. No atomic decides anything: the atomic OR that sets the bitmap bits is only
//       issued by the winners, whose points are distinct.
//   localmap_apply_kernel     an update: copies up to two runs of words from the staging block into the map's arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "localmap.h"

#pragma clang fp contract(off)      // every product and sum rounds on its own, as the restatement and the host function evaluate them

namespace dsdtm {

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_WAVES = LM_THREADS / 64;
constexpr unsigned long long LM_NOT_CLOSE = ~0ull;

// cvRound of a cv::Point2f member: narrowed to float first, then half to even (track.hip: cv_round / in_image)
__device__ __forceinline__ int lm_cv_round(double v) { return (int)rint((double)(float)v); }

__device__ __forceinline__ bool lm_in_image(int width, int height, double x, double y, int boundary) {   // src/Camera.cpp:187-193, level 0
    if (!(fabs(x) < 1e9) || !(fabs(y) < 1e9)) return false;
    const int xr = lm_cv_round(x), yr = lm_cv_round(y);
    return xr >= boundary && xr < width - boundary && yr >= boundary && yr < height - boundary;
}

__global__ __launch_bounds__(LM_THREADS) void localmap_visible_kernel(const LmSelectArgs a) {
    const LmDescDev* __restrict__ d = (const LmDescDev*)a.block + blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * LM_WAVES + wave;
    if (k >= d->K) return;                                  // (wave-uniform; the kernel has no barrier)
    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = d->T[i];
    const LmKeyframeDev* __restrict__ kf = d->kfs + k;
    const LmPointDev* __restrict__ pts = d->points;
    const int32_t* __restrict__ sl = d->slots + kf->slot_off;
    const int ns = kf->n_slots, P = d->P;
    const double fx = (double)a.fx, fy = (double)a.fy, cx = (double)a.cx, cy = (double)a.cy;
    bool hit = false;
    for (int base = 0; base < ns && !hit; base += 64) {
        const int i = base + lane;
        bool vis = false;
        const int p = i < ns ? sl[i] : -1;
        if (p >= 0 && p < P) {                              // :324 (p < P: the host checked every slot when it was written)
            const double X0 = pts[p].x, X1 = pts[p].y, X2 = pts[p].z;
            if (!(X0 == 0.0 && X1 == 0.0 && X2 == 0.0)) {   // :327 isZero(0)
                const double x = m[0] * X0 + m[1] * X1 + m[2] * X2 + m[3], y = m[4] * X0 + m[5] * X1 + m[6] * X2 + m[7],
                             z = m[8] * X0 + m[9] * X1 + m[10] * X2 + m[11];
                if (!(z < 0.0)) {                           // src/Frame.cpp:303
                    const double u = fx * x / z + cx, v = fy * y / z + cy;
                    vis = lm_in_image(a.width, a.height, u, v, a.boundary);
                }
            }
        }
        hit = __ballot(vis) != 0ull;
    }
    if (lane == 0) {
        unsigned long long key = LM_NOT_CLOSE;
        if (hit) {                                          // :333, Eigen's 3-vector reduction p0 + (p1 + p2)
            const double dx = m[3] - kf->T[3], dy = m[7] - kf->T[7], dz = m[11] - kf->T[11];
            key = (unsigned long long)__double_as_longlong(sqrt(dx * dx + (dy * dy + dz * dz)));
        }
        ((unsigned long long*)(a.block + d->keys))[k] = key;
    }
}

// LDS of the select kernel, all of it in the dynamic region: the fixed part, then the seen-bitmap (one bit per map point)
struct LmSelectLds {
    unsigned long long red_key[LM_WAVES];
    int red_idx[LM_WAVES];
    int wsum[LM_WAVES];
    int chosen[DSDTM_LOCALMAP_MAX_LOCAL];
    int chunk[LM_THREADS];
};
static_assert(sizeof(LmSelectLds) % 16 == 0, "the bitmap behind it stays 16-byte aligned");
static_assert(offsetof(LmSelectLds, chunk) % 16 == 0, "chunk[] is read four entries at a time");

__host__ __device__ inline size_t lm_bitmap_words(int P) { return ((size_t)(P > 0 ? P : 0) + 31) / 32; }

__global__ __launch_bounds__(LM_THREADS) void localmap_select_kernel(const LmSelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lm_lds[];
    LmSelectLds& s = *(LmSelectLds*)lm_lds;
    uint32_t* seen = (uint32_t*)(lm_lds + sizeof(LmSelectLds));
    const LmDescDev* __restrict__ d = (const LmDescDev*)a.block + blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = d->K, P = min(d->P, a.max_P), cap = d->capacity;
    const int n_local = min(max(a.n_local, 1), DSDTM_LOCALMAP_MAX_LOCAL);      // (the host checked; it bounds s.chosen)
    const unsigned long long* __restrict__ keys = (const unsigned long long*)(a.block + d->keys);
    double* kf_dist = (double*)(a.block + d->kf_dist);
    int32_t* kf_out = (int32_t*)(a.block + d->kf);
    int32_t* point = (int32_t*)(a.block + d->point);
    int32_t* point_kf = (int32_t*)(a.block + d->point_kf);

    for (size_t w = tid; w < lm_bitmap_words(P); w += LM_THREADS) seen[w] = 0u;

    // L3: the n_local smallest (key, index) pairs, one per round: the smallest pair above the one chosen last
    unsigned long long prev_key = 0ull;
    int prev_idx = -1, n_kf = 0, n_close = 0;
    for (int r = 0; r < n_local; ++r) {
        unsigned long long best_key = LM_NOT_CLOSE;
        int best_idx = 0x7fffffff, close = 0;
        for (int k = tid; k < K; k += LM_THREADS) {
            const unsigned long long key = keys[k];
            if (key == LM_NOT_CLOSE) continue;
            close += r == 0 ? 1 : 0;                        // (n_close is counted by the first round alone)
            const bool above = key > prev_key || (key == prev_key && k > prev_idx);
            if (above && key < best_key) { best_key = key; best_idx = k; }      // (k ascends: the first of equal keys stays)
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(best_key, o, 64);
            const int oi = __shfl_xor(best_idx, o, 64);
            if (ok < best_key || (ok == best_key && oi < best_idx)) { best_key = ok; best_idx = oi; }
            close += __shfl_xor(close, o, 64);
        }
        if (lane == 0) { s.red_key[wave] = best_key; s.red_idx[wave] = best_idx; s.wsum[wave] = close; }
        __syncthreads();
        best_key = s.red_key[0]; best_idx = s.red_idx[0]; close = s.wsum[0];
#pragma unroll
        for (int w = 1; w < LM_WAVES; ++w) {
            const unsigned long long ok = s.red_key[w];
            const int oi = s.red_idx[w];
            if (ok < best_key || (ok == best_key && oi < best_idx)) { best_key = ok; best_idx = oi; }
            close += s.wsum[w];
        }
        if (r == 0) n_close = close;
        __syncthreads();                                    // (the next round overwrites the partials)
        if (best_key == LM_NOT_CLOSE) break;                // workgroup-uniform: no close keyframe is left
        if (tid == 0) { s.chosen[r] = best_idx; kf_out[r] = best_idx; kf_dist[r] = __longlong_as_double((long long)best_key); }
        prev_key = best_key; prev_idx = best_idx;
        n_kf = r + 1;
    }
    __syncthreads();

    // L4: the walk
    const unsigned long long below = (1ull << lane) - 1ull;
    int n_points = 0;
    for (int j = 0; j < n_kf; ++j) {
        const LmKeyframeDev* __restrict__ kf = d->kfs + s.chosen[j];
        const int32_t* __restrict__ sl = d->slots + kf->slot_off;
        const int ns = kf->n_slots;
        for (int base = 0; base < ns; base += LM_THREADS) {
            const int i = base + tid;
            const int p = i < ns ? sl[i] : -1;
            // :288 NULL slot, :291 bad point, :294 already projected by an earlier chunk
            const bool cand = p >= 0 && p < P && d->points[p].bad == 0ull && ((seen[p >> 5] >> (p & 31)) & 1u) == 0u;
            s.chunk[tid] = cand ? p : -1;
            __syncthreads();
            bool emit = cand;
            if (cand) {                                     // :294 already projected by an earlier entry of this chunk (four per LDS read)
                const int4* c4 = (const int4*)s.chunk;
                for (int q = 0; q < (tid >> 2); ++q) {
                    const int4 v = c4[q];
                    emit = emit && v.x != p && v.y != p && v.z != p && v.w != p;
                }
                for (int q = tid & ~3; q < tid; ++q) emit = emit && s.chunk[q] != p;
            }
            if (emit) atomicOr(&seen[p >> 5], 1u << (p & 31));
            const unsigned long long mask = __ballot(emit);
            if (lane == 0) s.wsum[wave] = __popcll(mask);
            __syncthreads();
            int pos = n_points + __popcll(mask & below), total = 0;
#pragma unroll
            for (int w = 0; w < LM_WAVES; ++w) {
                if (w < wave) pos += s.wsum[w];
                total += s.wsum[w];
            }
            if (emit && pos < cap) { point[pos] = p; point_kf[pos] = j; }
            n_points += total;
            __syncthreads();                                // (the bitmap bits are set, chunk[] and wsum[] are free)
        }
    }
    if (tid == 0) {
        dsdtm_localmap_result res;
        res.n_close = n_close; res.n_kf = n_kf; res.n_points = n_points; res.overflow = n_points > cap ? 1 : 0;
        *(dsdtm_localmap_result*)(a.block + d->result) = res;
    }
}

__global__ __launch_bounds__(LM_THREADS) void localmap_apply_kernel(const LmApplyArgs a) {
    const uint32_t i = blockIdx.x * LM_THREADS + threadIdx.x;
    if (i < a.words[0]) a.dst[0][i] = a.src[0][i];
    if (i < a.words[1]) a.dst[1][i] = a.src[1][i];
}

}  // namespace

hipError_t localmap_apply_launch(const LmApplyArgs& args, hipStream_t stream) {
    const uint32_t words = args.words[0] > args.words[1] ? args.words[0] : args.words[1];
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(localmap_apply_kernel, dim3((words + LM_THREADS - 1) / LM_THREADS), dim3(LM_THREADS), 0, stream, args);
    return hipGetLastError();
}

hipError_t localmap_select_launch(const LmSelectArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const size_t lds = sizeof(LmSelectLds) + (lm_bitmap_words(args.max_P) * 4 + 15) / 16 * 16;
    if (lds > 64 * 1024) {      // more than 64 KB of dynamic LDS is an opt-in per kernel and device; harmless to repeat
        hipError_t e = hipFuncSetAttribute((const void*)localmap_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (args.max_K > 0) {
        hipLaunchKernelGGL(localmap_visible_kernel, dim3((unsigned)((args.max_K + LM_WAVES - 1) / LM_WAVES), (unsigned)args.n), dim3(LM_THREADS), 0,
                           stream, args);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(localmap_select_kernel, dim3((unsigned)args.n), dim3(LM_THREADS), lds, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
