// trackmap.hip — the flatten of dsdtm_trackmap_local (include/dsdtm_amd_trackmap.h): the points that the selection of localmap.hip left
// in the call's device block become dsdtm_track_desc's columns, with every observation of every emitted point, without a host round
// trip. Nothing here computes in floating point: every output is a copy.
//
//   trackmap_gather_kernel    one lane per emitted point: position, found count, bad flag; clears the point's counters.
//   trackmap_scan_kernel<0>   COUNT. The workgroups of a desc each load the desc's point -> list-position table into LDS (open
//       addressing, 8192 entries for at most 4096 points: load <= 0.5) and scan 64 keyframes of the map, one wavefront per
//       keyframe, lanes over its slots: ONE int32 per slot (the point index when the slot observes, -1 otherwise — an array of its
//       own, the feature columns are not touched). A hit adds 1 to count[position] (an integer atomic).
//   trackmap_offsets_kernel   one workgroup per desc: the exclusive prefix sum of count -> obs_offset, n_obs, overflow_obs, and the
//       point whose segment crosses obs_capacity, if any.
//   trackmap_scan_kernel<1>   FILL. The same scan; a hit of a point whose segment lies wholly below obs_capacity takes a cursor (an
//       integer atomic) and writes (keyframe << 32 | slot) there.
//   trackmap_straddle_kernel  only with overflow_obs: the segment that crosses obs_capacity gets its smallest keys, in order, by
//       repeated selection — what arrives first must not decide which of its observations are written. One workgroup per desc;
//       `want` rounds (the point's observations below obs_capacity), each a scan of the map's slots from the keyframe chosen last on:
//       at most want x slots / 256 loads per thread. It returns at once without overflow_obs.
//   trackmap_emit_kernel      one lane per written observation: its rank among the keys of its segment is its place (keys are
//       unique, so the order is ascending (keyframe, slot) whatever the arrival order was), and the lane copies the slot's pixel,
//       level and bearing there.
//   trackmap_apply_kernel / _points_kernel / _found_kernel: the updates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trackmap.h"

namespace dsdtm {

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_KF_PER_GROUP = 64;         // keyframes one workgroup of the scan covers
constexpr int TM_TABLE = 8192;              // entries of the LDS table (a power of two, twice DSDTM_TRACKMAP_MAX_LOCAL_POINTS)
constexpr int TM_PER_THREAD = DSDTM_TRACKMAP_MAX_LOCAL_POINTS / TM_THREADS;
static_assert(TM_TABLE >= 2 * DSDTM_TRACKMAP_MAX_LOCAL_POINTS && (TM_TABLE & (TM_TABLE - 1)) == 0, "load <= 0.5: a probe always ends");

struct TmView {
    const LmDescDev* ld;
    const TmDescDev* td;
    int m;                      // emitted points: min(n_points, point_capacity)
};
__device__ __forceinline__ TmView tm_view(const TmLocalArgs& a, unsigned t) {
    TmView v;
    v.ld = (const LmDescDev*)a.block + t;
    v.td = (const TmDescDev*)(a.block + a.descs) + t;
    const dsdtm_localmap_result* r = (const dsdtm_localmap_result*)(a.block + v.ld->result);
    v.m = min(max(r->n_points, 0), min(v.ld->capacity, DSDTM_TRACKMAP_MAX_LOCAL_POINTS));
    return v;
}

__device__ __forceinline__ unsigned tm_hash(int p) { return ((unsigned)p * 2654435761u) >> 19; }      // 13 bits

__global__ __launch_bounds__(TM_THREADS) void trackmap_gather_kernel(const TmLocalArgs a) {
    const TmView v = tm_view(a, blockIdx.y);
    const int i = (int)blockIdx.x * TM_THREADS + (int)threadIdx.x;
    if (i < v.ld->capacity) {
        ((int32_t*)(a.block + v.td->count))[i] = 0;
        ((int32_t*)(a.block + v.td->cursor))[i] = 0;
    }
    if (i >= v.m) return;
    const int p = ((const int32_t*)(a.block + v.ld->point))[i];
    if (p < 0 || p >= v.ld->P) return;                      // (the selection emits points of the map only)
    const LmPointDev pt = v.ld->points[p];
    double* w = (double*)(a.block + v.td->mp_world) + 3 * (size_t)i;
    w[0] = pt.x; w[1] = pt.y; w[2] = pt.z;
    ((int32_t*)(a.block + v.td->mp_found))[i] = v.td->found[p];
    ((uint8_t*)(a.block + v.td->mp_bad))[i] = pt.bad ? 1 : 0;
}

template <bool FILL>
__global__ __launch_bounds__(TM_THREADS) void trackmap_scan_kernel(const TmLocalArgs a) {
    __shared__ int32_t t_key[TM_TABLE];
    __shared__ uint16_t t_pos[TM_TABLE];
    const TmView v = tm_view(a, blockIdx.y);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = v.ld->K, k0 = (int)blockIdx.x * TM_KF_PER_GROUP;
    if (k0 >= K || v.m == 0) return;                        // (workgroup-uniform, in front of every barrier)
    for (int e = tid; e < TM_TABLE; e += TM_THREADS) t_key[e] = -1;
    __syncthreads();
    const int32_t* __restrict__ point = (const int32_t*)(a.block + v.ld->point);
    for (int i = tid; i < v.m; i += TM_THREADS) {           // the emitted points are distinct (rule L4): each claims one entry
        const int p = point[i];
        unsigned h = tm_hash(p);
        while (atomicCAS(&t_key[h], -1, p) != -1) h = (h + 1) & (TM_TABLE - 1);
        t_pos[h] = (uint16_t)i;
    }
    __syncthreads();
    int32_t* count = (int32_t*)(a.block + v.td->count);
    int32_t* cursor = (int32_t*)(a.block + v.td->cursor);
    const int32_t* off = (const int32_t*)(a.block + v.td->obs_offset);
    unsigned long long* pairs = (unsigned long long*)(a.block + v.td->pairs);
    const int ocap = v.td->ocap;
    for (int kk = wave; kk < TM_KF_PER_GROUP; kk += TM_WAVES) {
        const int k = k0 + kk;
        if (k >= K) break;
        const LmKeyframeDev* __restrict__ kf = v.ld->kfs + k;
        const int32_t* __restrict__ ob = v.td->obs + kf->slot_off;
        const int ns = kf->n_slots;
        for (int s = lane; s < ns; s += 64) {
            const int p = ob[s];
            if (p < 0) continue;
            unsigned h = tm_hash(p);
            int i = -1;
            for (int q = t_key[h]; q != -1; q = t_key[h]) {
                if (q == p) { i = t_pos[h]; break; }
                h = (h + 1) & (TM_TABLE - 1);
            }
            if (i < 0) continue;
            if (!FILL) {
                atomicAdd(&count[i], 1);
            } else if (off[i + 1] <= ocap) {                // a segment wholly below obs_capacity (the crossing one: the straddle kernel)
                const int j = off[i] + atomicAdd(&cursor[i], 1);
                if (j < off[i + 1]) pairs[j] = ((unsigned long long)(unsigned)k << 32) | (unsigned)s;
            }
        }
    }
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_offsets_kernel(const TmLocalArgs a) {
    __shared__ int wsum[TM_WAVES];
    __shared__ int straddle;
    const TmView v = tm_view(a, blockIdx.x);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t* count = (const int32_t*)(a.block + v.td->count);
    int32_t* off = (int32_t*)(a.block + v.td->obs_offset);
    const int ocap = v.td->ocap;
    int c[TM_PER_THREAD], mine = 0;
#pragma unroll
    for (int e = 0; e < TM_PER_THREAD; ++e) {
        const int i = tid * TM_PER_THREAD + e;
        c[e] = i < v.m ? count[i] : 0;
        mine += c[e];
    }
    int incl = mine;                                        // inclusive scan over the wavefront, then over the four wavefronts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    if (tid == 0) straddle = -1;
    __syncthreads();
    int base = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < TM_WAVES; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
#pragma unroll
    for (int e = 0; e < TM_PER_THREAD; ++e) {
        const int i = tid * TM_PER_THREAD + e;
        if (i < v.m) {
            off[i] = base;
            if (base < ocap && base + c[e] > ocap) straddle = i;      // (at most one point)
        }
        base += c[e];
    }
    if (tid == 0) off[v.m] = total;
    __syncthreads();
    if (tid == 0) {
        TmExtResult r;
        r.n_obs = total; r.overflow_obs = total > ocap ? 1 : 0; r.straddle = straddle; r.reserved = 0;
        *(TmExtResult*)(a.block + v.td->ext) = r;
    }
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_straddle_kernel(const TmLocalArgs a) {
    __shared__ unsigned long long best;
    const TmView v = tm_view(a, blockIdx.x);
    const int i = ((const TmExtResult*)(a.block + v.td->ext))->straddle;
    if (i < 0 || i >= v.m) return;                          // (workgroup-uniform)
    const int tid = threadIdx.x;
    const int p = ((const int32_t*)(a.block + v.ld->point))[i];
    const int a0 = ((const int32_t*)(a.block + v.td->obs_offset))[i], want = v.td->ocap - a0;      // fewer than the segment holds
    unsigned long long* pairs = (unsigned long long*)(a.block + v.td->pairs);
    const int K = v.ld->K;
    unsigned long long prev = 0ull;
    for (int t = 0; t < want; ++t) {                        // the smallest key above the one chosen last
        if (tid == 0) best = ~0ull;
        __syncthreads();
        unsigned long long mine = ~0ull;
        for (int k = (int)(prev >> 32); k < K && mine == ~0ull; ++k) {      // (keys ascend with k: a thread stops at its first)
            const LmKeyframeDev* __restrict__ kf = v.ld->kfs + k;
            const int32_t* __restrict__ ob = v.td->obs + kf->slot_off;
            for (int s = tid; s < kf->n_slots; s += TM_THREADS) {
                const unsigned long long key = ((unsigned long long)(unsigned)k << 32) | (unsigned)s;
                if (ob[s] == p && (t == 0 || key > prev)) { mine = key; break; }
            }
        }
        if (mine != ~0ull) atomicMin(&best, mine);
        __syncthreads();
        prev = best;
        if (tid == 0) pairs[a0 + t] = prev;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_emit_kernel(const TmLocalArgs a) {
    const TmView v = tm_view(a, blockIdx.y);
    const int j = (int)blockIdx.x * TM_THREADS + (int)threadIdx.x;
    const int32_t* __restrict__ off = (const int32_t*)(a.block + v.td->obs_offset);
    if (v.m == 0) return;
    const int lim = min(off[v.m], v.td->ocap);
    if (j >= lim) return;
    int lo = 0, hi = v.m;                                   // the last point whose offset is <= j: the segment j lies in
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    const int s0 = off[lo], s1 = min(off[lo + 1], lim);
    const unsigned long long* __restrict__ pairs = (const unsigned long long*)(a.block + v.td->pairs);
    const unsigned long long me = pairs[j];
    int rank = 0;
    for (int q = s0; q < s1; ++q) rank += pairs[q] < me ? 1 : 0;
    const int o = s0 + rank, k = (int)(me >> 32), s = (int)(me & 0xffffffffull);
    if ((unsigned)k >= (unsigned)v.ld->K || (unsigned)s >= (unsigned)v.ld->kfs[k].n_slots) return;      // (keys are (keyframe, slot) pairs of the map)
    const TmFeatDev f = v.td->feat[v.ld->kfs[k].slot_off + s];
    ((int32_t*)(a.block + v.td->obs_kf))[o] = k;
    float* px = (float*)(a.block + v.td->obs_px) + 2 * (size_t)o;
    px[0] = f.px[0]; px[1] = f.px[1];
    ((int32_t*)(a.block + v.td->obs_level))[o] = f.level;
    double* b = (double*)(a.block + v.td->obs_bearing) + 3 * (size_t)o;
    b[0] = f.bearing[0]; b[1] = f.bearing[1]; b[2] = f.bearing[2];
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_apply_kernel(const TmApplyArgs a) {
    const uint32_t i = blockIdx.x * TM_THREADS + threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (i < a.words[r]) a.dst[r][i] = a.src[r][i];
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_points_kernel(const TmPointsArgs a) {
    const int i = (int)(blockIdx.x * TM_THREADS + threadIdx.x);
    if (i >= a.n) return;
    const int idx = a.first + i;
    LmPointDev* pt = a.points + idx;
    pt->x = a.xyz[3 * (size_t)i]; pt->y = a.xyz[3 * (size_t)i + 1]; pt->z = a.xyz[3 * (size_t)i + 2];
    if (a.bad) pt->bad = a.bad[i] ? 1ull : 0ull;
    else if (idx >= a.old_count) pt->bad = 0ull;
    if (a.found) a.found_dst[idx] = a.found[i];
    else if (idx >= a.old_count) a.found_dst[idx] = 0;
}

__global__ __launch_bounds__(TM_THREADS) void trackmap_found_kernel(int32_t* found_dst, const int32_t* index, const int32_t* found, int n) {
    const int i = (int)(blockIdx.x * TM_THREADS + threadIdx.x);
    if (i < n) found_dst[index[i]] = found[i];
}

inline unsigned tm_groups(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t trackmap_apply_launch(const TmApplyArgs& args, hipStream_t stream) {
    uint32_t words = 0;
    for (int r = 0; r < 4; ++r) words = args.words[r] > words ? args.words[r] : words;
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(trackmap_apply_kernel, dim3(tm_groups(words, TM_THREADS)), dim3(TM_THREADS), 0, stream, args);
    return hipGetLastError();
}

hipError_t trackmap_points_launch(const TmPointsArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(trackmap_points_kernel, dim3(tm_groups(args.n, TM_THREADS)), dim3(TM_THREADS), 0, stream, args);
    return hipGetLastError();
}

hipError_t trackmap_found_launch(int32_t* found_dst, const int32_t* index, const int32_t* found, int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(trackmap_found_kernel, dim3(tm_groups(n, TM_THREADS)), dim3(TM_THREADS), 0, stream, found_dst, index, found, n);
    return hipGetLastError();
}

hipError_t trackmap_flatten_launch(const TmLocalArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)args.n;
    hipError_t e;
    hipLaunchKernelGGL(trackmap_gather_kernel, dim3(tm_groups(args.max_cap > 0 ? args.max_cap : 1, TM_THREADS), n), dim3(TM_THREADS), 0, stream, args);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (args.max_K > 0 && args.max_cap > 0) {
        hipLaunchKernelGGL(trackmap_scan_kernel<false>, dim3(tm_groups(args.max_K, TM_KF_PER_GROUP), n), dim3(TM_THREADS), 0, stream, args);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(trackmap_offsets_kernel, dim3(n), dim3(TM_THREADS), 0, stream, args);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (args.max_K > 0 && args.max_cap > 0 && args.max_ocap > 0) {
        hipLaunchKernelGGL(trackmap_scan_kernel<true>, dim3(tm_groups(args.max_K, TM_KF_PER_GROUP), n), dim3(TM_THREADS), 0, stream, args);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(trackmap_straddle_kernel, dim3(n), dim3(TM_THREADS), 0, stream, args);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(trackmap_emit_kernel, dim3(tm_groups(args.max_ocap, TM_THREADS), n), dim3(TM_THREADS), 0, stream, args);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsdtm
