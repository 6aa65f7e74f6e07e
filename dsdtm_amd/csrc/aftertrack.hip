// aftertrack.hip — what follows PoseOptimization on every tracked frame, on the resident map, for gfx950 (include/dsdtm_amd_slam.h).
// dsdtm_slam_track_commit (rules T1-T4):
//   aftertrack_walk_kernel     one 256-thread workgroup per DISTINCT map of the call. It first clears the map's stamp bytes (one per
//       point, in the call's block), then walks the map's descs in desc order (T4), thread k owning match k. Per desc: T1
//       (found += 1), a barrier, T2 (the erase with the bad transition: bad = 1 and stamp = 1), then the newly-bad points are appended in
//       MATCH order — a ballot per wavefront, the wavefronts' counts through LDS — to the desc's bad list. A desc names each point
//       once (the host checked), so within a desc every point has one owner; the barriers between descs order the owners of one
//       point across descs. Every thread runs every iteration up to the barriers: the trip count is the map's desc count.
//   aftertrack_cascade_kernel  behind it on the same stream, one thread per slot of each map's pool. A block whose map gained no bad
//       point returns at once (the device decides: nothing waits in between). A slot whose observing point carries the stamp gets
//       obs = -1 and point_of_slot = -1 (T3): one byte load per observing slot, whatever the number of points that went bad. The
//       stamp is "went bad IN THIS CALL", distinct from `bad`: a point that was bad before keeps its slots; a slot that lists a point
//       without observing it has obs = -1 and is never looked at.
// dsdtm_slam_need_keyframes:
//   aftertrack_gather_kernel   one 256-thread workgroup per tracker builds, in the call's block, what dsdtm_need_keyframes uploads:
//       the current frame's points and flags from their map indices, the last keyframe's pose and its listed slots compacted in
//       SLOT order (ballot prefix, 256 slots per round, a running base), the local keyframes' camera centres
//       c_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2) with separate multiplies and adds (__dmul_rn / __dadd_rn: never contracted).
//       keyframe.hip's kernel follows on the stream, unchanged.
// No kernel waits for another workgroup; nothing is ordered by an atomic's arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aftertrack.h"

namespace dsdtm {
namespace {

constexpr int AT_WAVES = AT_THREADS / 64;

__global__ __launch_bounds__(AT_THREADS) void aftertrack_walk_kernel(AtCommitArgs a) {
    __shared__ int32_t s_bad[AT_WAVES], s_erased[AT_WAVES];
    const AtMapDev m = ((const AtMapDev*)a.block)[blockIdx.x];
    const AtDescDev* descs = (const AtDescDev*)(a.block + a.descs);
    const int32_t* list = (const int32_t*)(a.block + m.desc_list);
    uint8_t* stamp = a.block + m.stamp;
    const int k = (int)threadIdx.x, lane = k & 63, wave = k >> 6;
    for (int w = k; w < (m.P + 3) / 4; w += AT_THREADS) ((uint32_t*)stamp)[w] = 0u;       // (room: P rounded up to 8)
    __syncthreads();
    int total_bad = 0;                                  // uniform: every thread adds every desc's count
    for (int di = 0; di < m.n_descs; ++di) {
        const AtDescDev d = descs[list[di]];
        int p = -1;
        if (k < d.n_matches) {
            p = ((const int32_t*)(a.block + d.point))[k];
            if (p < 0 || p >= m.P) p = -1;              // (the host refused such a call: never taken)
        }
        int f = 0;
        if (p >= 0) { f = m.found[p] + 1; m.found[p] = f; }                     // T1
        __syncthreads();
        bool erased = false, went_bad = false;
        if (p >= 0) {                                                           // T2: this thread is the point's only owner in this desc
            const double norm = ((const double*)(a.block + d.norm))[k];
            if (norm > a.threshold && m.points[p].bad == 0) {
                erased = true;
                f -= 1;
                m.found[p] = f;
                if (f <= 0) { went_bad = true; m.points[p].bad = 1ull; stamp[p] = 1; }
            }
            ((int32_t*)(a.block + d.found_after))[k] = f;
        }
        const unsigned long long bad_mask = __ballot(went_bad), erased_mask = __ballot(erased);
        if (lane == 0) { s_bad[wave] = __popcll(bad_mask); s_erased[wave] = __popcll(erased_mask); }
        __syncthreads();
        int before = 0, n_bad = 0, n_erased = 0;
        for (int w = 0; w < AT_WAVES; ++w) {
            if (w < wave) before += s_bad[w];
            n_bad += s_bad[w];
            n_erased += s_erased[w];
        }
        if (went_bad) {
            const int rank = before + __popcll(bad_mask & ((1ull << lane) - 1ull));
            if (rank < d.bad_cap) ((int32_t*)(a.block + d.bad_list))[rank] = p;
        }
        if (k == 0) {
            dsdtm_slam_commit_result r;
            r.n_erased = n_erased; r.n_bad = n_bad; r.overflow_bad = 0; r.reserved = 0;     // (overflow_bad: the host, which knows bad_capacity)
            *(dsdtm_slam_commit_result*)(a.block + d.result) = r;
        }
        total_bad += n_bad;
        __syncthreads();                                // the next desc's owners see this desc's counts and flags; s_* are free again
    }
    if (k == 0) *(int32_t*)(a.block + m.n_new_bad) = total_bad;
}

__global__ __launch_bounds__(AT_THREADS) void aftertrack_cascade_kernel(AtCommitArgs a) {
    const AtMapDev m = ((const AtMapDev*)a.block)[blockIdx.y];
    if (*(const int32_t*)(a.block + m.n_new_bad) <= 0) return;
    const long long s = (long long)blockIdx.x * AT_THREADS + threadIdx.x;
    if (s >= m.S) return;
    const int p = m.obs[s];
    if (p < 0 || p >= m.P) return;
    if ((a.block + m.stamp)[p]) {
        m.obs[s] = -1;
        m.slots[s] = -1;
    }
}

__global__ __launch_bounds__(AT_THREADS) void aftertrack_gather_kernel(AtGatherArgs a) {
    __shared__ int32_t s_count[AT_WAVES];
    const int t = (int)blockIdx.x, k = (int)threadIdx.x, lane = k & 63, wave = k >> 6;
    KeyframeTrackerDev* rec = (KeyframeTrackerDev*)a.block + t;
    const AtGatherDev g = ((const AtGatherDev*)(a.block + a.descs))[t];
    const int n_cur = rec->n_cur, n_lkf = rec->n_lkf;
    // the current frame's points
    const int32_t* cur_point = (const int32_t*)(a.block + g.cur_point);
    double* cur_p = (double*)(a.block + rec->cur_p);
    uint8_t* cur_bad = a.block + rec->cur_bad;
    for (int i = k; i < n_cur; i += AT_THREADS) {
        const int p = cur_point[i];
        if (p < 0 || p >= g.P) continue;                // (the host refused such a call: never taken)
        const LmPointDev pt = g.points[p];
        cur_p[3 * i] = pt.x; cur_p[3 * i + 1] = pt.y; cur_p[3 * i + 2] = pt.z;
        cur_bad[i] = pt.bad ? 1 : 0;
    }
    // the local keyframes' camera centres
    const int32_t* local_kf = (const int32_t*)(a.block + g.local_kf);
    double* lkf = (double*)(a.block + rec->lkf);
    for (int i = k; i < n_lkf; i += AT_THREADS) {
        const int q = local_kf[i];
        if (q < 0 || q >= g.K) continue;
        const double* T = g.kfs[q].T;
        for (int c = 0; c < 3; ++c)
            lkf[3 * i + c] = -__dadd_rn(__dadd_rn(__dmul_rn(T[c], T[3]), __dmul_rn(T[4 + c], T[7])), __dmul_rn(T[8 + c], T[11]));
    }
    // the last keyframe: its pose, and its listed slots in slot order
    const LmKeyframeDev* kf = g.kfs + g.kf;
    if (k < 12) rec->T_kf[k] = kf->T[k];
    const int n_slots = kf->n_slots;
    const int32_t* slots = g.slots + kf->slot_off;
    double* kf_p = (double*)(a.block + rec->kf_p);
    uint8_t* kf_bad = a.block + rec->kf_bad;
    int base = 0;                                       // uniform
    for (int s0 = 0; s0 < n_slots; s0 += AT_THREADS) {  // (uniform trip count: every thread reaches both barriers)
        const int s = s0 + k;
        int p = s < n_slots ? slots[s] : -1;
        if (p >= g.P) p = -1;
        const unsigned long long mask = __ballot(p >= 0);
        if (lane == 0) s_count[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < AT_WAVES; ++w) {
            if (w < wave) before += s_count[w];
            total += s_count[w];
        }
        if (p >= 0) {
            const int o = base + before + __popcll(mask & ((1ull << lane) - 1ull));      // (o < n_slots: the room of kf_p and kf_bad)
            const LmPointDev pt = g.points[p];
            kf_p[3 * o] = pt.x; kf_p[3 * o + 1] = pt.y; kf_p[3 * o + 2] = pt.z;
            kf_bad[o] = pt.bad ? 1 : 0;
        }
        base += total;
        __syncthreads();
    }
    if (k == 0) rec->n_kf = base;
}

}  // namespace

hipError_t aftertrack_commit_launch(const AtCommitArgs& args, hipStream_t stream) {
    if (args.n_maps <= 0) return hipSuccess;
    hipLaunchKernelGGL(aftertrack_walk_kernel, dim3((unsigned)args.n_maps), dim3(AT_THREADS), 0, stream, args);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || args.max_S <= 0) return e;
    const unsigned blocks = (unsigned)((args.max_S + AT_THREADS - 1) / AT_THREADS);
    hipLaunchKernelGGL(aftertrack_cascade_kernel, dim3(blocks, (unsigned)args.n_maps), dim3(AT_THREADS), 0, stream, args);
    return hipGetLastError();
}

hipError_t aftertrack_gather_launch(const AtGatherArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(aftertrack_gather_kernel, dim3((unsigned)args.n), dim3(AT_THREADS), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
