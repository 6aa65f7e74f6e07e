// mapping.hip — the kernels of libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h): the covisibility list of KeyFrame::UpdateConnection,
// the window of Optimizer::LocalBundleAdjustment and the commit of its solve, on the resident track map. Nothing here computes in
// floating point: every value written is a copy. Every ORDER comes from keys — (rank of the local keyframe, slot), (window point,
// keyframe), (keyframe, slot) — never from which lane arrived first: the atomics below are integer sums, minima and maxima, whose
// results do not depend on the order of arrival. A value that atomics of SEVERAL workgroups produced in global memory is read by a
// LATER launch only; within a launch only LDS atomics are read back (behind a barrier), and the value an atomicCAS returns steers
// nothing but its own lane's probe.
//
//   covisibility   mapping_cov_weight_kernel   a workgroup per 64 keyframes of a pair's map: the listed, non-bad points of `kf` with
//                      their multiplicity in an LDS table (<= 4096 slots, 8192 entries); one wavefront per keyframe sums the
//                      multiplicities of its observing slots and stores the keyframe's weight (no atomic: one writer).
//                  mapping_cov_list_kernel     one workgroup per pair: the counts, the fallback keyframe, and each listed keyframe's
//                      rank among the listed ones by (weight, index).
//   window         mapping_win_init_kernel     the temporaries of the call's block.
//                  mapping_win_insert_kernel   one lane per ENTRY (a slot of a local keyframe): the first-occurrence table in the
//                      call's block gets (point << 32 | entry) by atomicMin — the smallest entry that lists a point, whoever comes first.
//                  mapping_win_first_kernel    one workgroup per window, entries in order: an entry that finds itself in the table is
//                      a first occurrence; an exclusive scan over the flags numbers the window's points (W2).
//                  mapping_win_count_kernel    the map's observing slots, one wavefront per keyframe: a slot of a window point adds 1
//                      to the point's count, and a keyframe that is not local takes the minimum of the window points it observes:
//                      its place among the fixed keyframes is the rank of (that minimum, keyframe index) (W3).
//                  mapping_win_offsets_kernel  one workgroup per window: the fixed keyframes by rank, the poses, the prefix sum of the
//                      counts, the flags and the result.
//                  mapping_win_fill_kernel / _emit_kernel   usable windows only: the keys (keyframe << 32 | slot) of each point's
//                      segment, then each observation at the rank of its key within the segment (W4).
//   commit         mapping_commit_claim / _verify_kernel    every keyframe and point of every usable window claims its map entry by
//                      atomicMin of the window's number; an entry that another window holds is an overlap, and the smallest
//                      (holder, window) pair is the verdict the host waits for. Nothing of the map is written.
//                  mapping_commit_apply_kernel one lane per window keyframe (the pose) and per window point (the position and the
//                      outlier pass of that point, in observation order: C1, C2).
//                  mapping_commit_collect_kernel   one workgroup per window: the counts and the points that went bad, in window order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapping.h"

namespace dsdtm {

namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_KF_PER_GROUP = 64;
constexpr int MP_COV_TABLE = 8192;
constexpr unsigned long long MP_EMPTY = ~0ull;
constexpr int MP_NONE = 0x7fffffff;
static_assert(MP_COV_TABLE >= 2 * DSDTM_LOCALMAP_MAX_SLOTS && (MP_COV_TABLE & (MP_COV_TABLE - 1)) == 0, "load <= 0.5: a probe always ends");

inline unsigned mp_groups(long long n, int per) { return (unsigned)((n > 0 ? n : 1) + per - 1) / per; }

// the exclusive prefix sum of one int per thread over the workgroup; total = the sum (two barriers; wsum: MP_WAVES ints of LDS)
__device__ __forceinline__ int mp_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < MP_WAVES; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    return base;
}

// ---------------------------------------------------------------------------------------------------------------- covisibility

__device__ __forceinline__ unsigned mp_hash13(int p) { return ((unsigned)p * 2654435761u) >> 19; }

__global__ __launch_bounds__(MP_THREADS) void mapping_cov_weight_kernel(const MpCovArgs a) {
    __shared__ int32_t t_key[MP_COV_TABLE];
    __shared__ uint32_t t_cnt[MP_COV_TABLE / 2];            // 16 bits per entry (a count is at most 4096)
    const MpCovDev* d = (const MpCovDev*)a.block + blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = d->K, k0 = (int)blockIdx.x * MP_KF_PER_GROUP;
    if (k0 >= K) return;                                    // (workgroup-uniform, in front of every barrier)
    for (int e = tid; e < MP_COV_TABLE; e += MP_THREADS) t_key[e] = -1;
    for (int e = tid; e < MP_COV_TABLE / 2; e += MP_THREADS) t_cnt[e] = 0u;
    __syncthreads();
    const LmKeyframeDev* me = d->kfs + d->kf;
    const int32_t* __restrict__ mine = d->slots + me->slot_off;
    const int ns = min(me->n_slots, DSDTM_LOCALMAP_MAX_SLOTS);
    for (int s = tid; s < ns; s += MP_THREADS) {
        const int p = mine[s];
        if (p < 0 || d->points[p].bad) continue;
        unsigned h = mp_hash13(p);
        for (;;) {
            const int old = atomicCAS(&t_key[h], -1, p);
            if (old == -1 || old == p) break;
            h = (h + 1) & (MP_COV_TABLE - 1);
        }
        atomicAdd(&t_cnt[h >> 1], (h & 1u) ? 0x10000u : 1u);
    }
    __syncthreads();
    int32_t* weight = (int32_t*)(a.block + d->weight);
    for (int kk = wave; kk < MP_KF_PER_GROUP; kk += MP_WAVES) {
        const int k = k0 + kk;
        if (k >= K) break;
        const LmKeyframeDev* __restrict__ kf = d->kfs + k;
        const int32_t* __restrict__ ob = d->obs + kf->slot_off;
        int sum = 0;
        if (k != d->kf)
            for (int s = lane; s < kf->n_slots; s += 64) {
                const int p = ob[s];
                if (p < 0) continue;
                unsigned h = mp_hash13(p);
                for (int q = t_key[h]; q != -1; q = t_key[h]) {
                    if (q == p) { sum += (int)((t_cnt[h >> 1] >> ((h & 1u) * 16)) & 0xffffu); break; }
                    h = (h + 1) & (MP_COV_TABLE - 1);
                }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        if (lane == 0) weight[k] = sum;
    }
}

__global__ __launch_bounds__(MP_THREADS) void mapping_cov_list_kernel(const MpCovArgs a) {
    __shared__ int s_conn, s_over;
    __shared__ unsigned long long s_best;
    const MpCovDev* d = (const MpCovDev*)a.block + blockIdx.x;
    const int tid = threadIdx.x, K = d->K, cap = d->capacity;
    const int32_t* __restrict__ weight = (const int32_t*)(a.block + d->weight);
    int32_t* cov_kf = (int32_t*)(a.block + d->cov_kf);
    int32_t* cov_w = (int32_t*)(a.block + d->cov_weight);
    if (tid == 0) { s_conn = 0; s_over = 0; s_best = 0ull; }
    __syncthreads();
    int conn = 0, over = 0;
    unsigned long long best = 0ull;                         // the largest weight; among equals the LOWEST index
    for (int k = tid; k < K; k += MP_THREADS) {
        const int w = weight[k];
        if (w <= 0) continue;
        ++conn;
        if (w > DSDTM_MAPPING_COV_THRESHOLD) ++over;
        const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (0xffffffffu - (unsigned)k);
        best = key > best ? key : best;
    }
    if (conn) { atomicAdd(&s_conn, conn); atomicMax(&s_best, best); }
    if (over) atomicAdd(&s_over, over);
    __syncthreads();
    const int n_conn = s_conn, n_over = s_over;
    int n_cov = 0;
    if (n_over > 0) {
        n_cov = n_over;
        for (int k = tid; k < K; k += MP_THREADS) {
            const int w = weight[k];
            if (w <= DSDTM_MAPPING_COV_THRESHOLD) continue;
            int rank = 0;                                   // ascending (weight, index)
            for (int q = 0; q < K; ++q) {
                const int wq = weight[q];
                rank += (wq > DSDTM_MAPPING_COV_THRESHOLD && (wq < w || (wq == w && q < k))) ? 1 : 0;
            }
            if (rank < cap) { cov_kf[rank] = k; cov_w[rank] = w; }
        }
    } else if (n_conn > 0) {
        n_cov = 1;
        if (tid == 0 && cap > 0) { cov_kf[0] = (int)(0xffffffffu - (unsigned)(s_best & 0xffffffffull)); cov_w[0] = (int)(s_best >> 32); }
    }
    if (tid == 0) {
        dsdtm_mapping_cov_result r;
        r.n_cov = n_cov; r.n_connected = n_conn; r.overflow = n_cov > cap ? 1 : 0; r.reserved = 0;
        *(dsdtm_mapping_cov_result*)(a.block + d->result) = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- window

__device__ __forceinline__ unsigned mp_hash(int p, int bits) { return ((unsigned)p * 2654435761u) >> (32 - bits); }

// the cell of point p in the first-occurrence table, or -1
__device__ __forceinline__ int mp_find(const unsigned long long* __restrict__ table, int bits, int p) {
    const unsigned mask = (1u << bits) - 1u;
    unsigned h = mp_hash(p, bits);
    for (;;) {
        const unsigned long long v = table[h];
        if (v == MP_EMPTY) return -1;
        if ((int)(v >> 32) == p) return (int)h;
        h = (h + 1) & mask;
    }
}

// the point entry e lists, if it takes part in W2 (set, in the map, not bad; none at all when kf == origin_kf), else -1
__device__ __forceinline__ int mp_entry_point(const MpWinDev* d, const uint8_t* block, int e) {
    if (d->kf == d->origin) return -1;
    const int32_t* __restrict__ ent_off = (const int32_t*)(block + d->ent_off);
    const int32_t* __restrict__ local = (const int32_t*)(block + d->local);
    int lo = 0, hi = d->n_local;                            // the last local keyframe whose first entry is <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ent_off[mid] <= e) lo = mid; else hi = mid;
    }
    const int p = d->slots[d->kfs[local[lo]].slot_off + (e - ent_off[lo])];
    if (p < 0 || p >= d->P || d->points[p].bad) return -1;
    return p;
}

__global__ __launch_bounds__(MP_THREADS) void mapping_win_init_kernel(const MpWinArgs a) {
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.y;
    const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
    if (i < (1ll << d->T_bits)) {
        ((unsigned long long*)(a.block + d->table))[i] = MP_EMPTY;
        ((int32_t*)(a.block + d->cell_lp))[i] = -1;
    }
    if (i < d->K) {
        ((int32_t*)(a.block + d->kfkey))[i] = MP_NONE;
        ((int32_t*)(a.block + d->kfwin))[i] = -1;
    }
    if (i < d->E) {
        ((int32_t*)(a.block + d->count))[i] = 0;
        ((int32_t*)(a.block + d->cursor))[i] = 0;
    }
}

__global__ __launch_bounds__(MP_THREADS) void mapping_win_insert_kernel(const MpWinArgs a) {
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.y;
    const int e = (int)blockIdx.x * MP_THREADS + (int)threadIdx.x;
    if (e < d->n_local) ((int32_t*)(a.block + d->kfwin))[((const int32_t*)(a.block + d->local))[e]] = e;      // (the host checked: distinct, below K)
    if (e >= d->E) return;
    const int p = mp_entry_point(d, a.block, e);
    if (p < 0) return;
    unsigned long long* table = (unsigned long long*)(a.block + d->table);
    const unsigned mask = (1u << d->T_bits) - 1u;
    const unsigned long long mine = ((unsigned long long)(unsigned)p << 32) | (unsigned)e;
    unsigned h = mp_hash(p, d->T_bits);
    for (;;) {
        const unsigned long long cur = atomicCAS(&table[h], MP_EMPTY, mine);
        if (cur == MP_EMPTY) break;
        if ((int)(cur >> 32) == p) { atomicMin(&table[h], mine); break; }
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(MP_THREADS) void mapping_win_first_kernel(const MpWinArgs a) {
    __shared__ int wsum[MP_WAVES];
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.x;
    const int tid = threadIdx.x, E = d->E;
    const unsigned long long* __restrict__ table = (const unsigned long long*)(a.block + d->table);
    int32_t* cell_lp = (int32_t*)(a.block + d->cell_lp);
    int run = 0;
    for (int base = 0; base < E; base += MP_THREADS) {      // (workgroup-uniform bounds)
        const int e = base + tid;
        int p = -1, h = -1, flag = 0;
        if (e < E) p = mp_entry_point(d, a.block, e);
        if (p >= 0) h = mp_find(table, d->T_bits, p);
        if (h >= 0 && (unsigned)(table[h] & 0xffffffffull) == (unsigned)e) flag = 1;
        int total;
        const int lp = run + mp_scan(flag, wsum, total);
        if (flag) {
            cell_lp[h] = lp;
            if (lp < d->pcap) {
                const LmPointDev pt = d->points[p];
                d->point_index[lp] = p;
                d->pts[3 * (size_t)lp] = pt.x; d->pts[3 * (size_t)lp + 1] = pt.y; d->pts[3 * (size_t)lp + 2] = pt.z;
            }
        }
        run += total;
    }
    if (tid == 0) ((dsdtm_mapping_window_result*)(a.block + d->result))->n_points = run;
}

template <bool FILL>
__global__ __launch_bounds__(MP_THREADS) void mapping_win_scan_kernel(const MpWinArgs a) {
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.y;
    const dsdtm_mapping_window_result* res = (const dsdtm_mapping_window_result*)(a.block + d->result);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = d->K, k0 = (int)blockIdx.x * MP_KF_PER_GROUP;
    if (k0 >= K || res->n_points == 0) return;
    if (FILL && !res->usable) return;
    const unsigned long long* __restrict__ table = (const unsigned long long*)(a.block + d->table);
    const int32_t* __restrict__ cell_lp = (const int32_t*)(a.block + d->cell_lp);
    const int32_t* __restrict__ kfwin = (const int32_t*)(a.block + d->kfwin);
    const int32_t* __restrict__ off = (const int32_t*)(a.block + d->off);
    int32_t* count = (int32_t*)(a.block + d->count);
    int32_t* cursor = (int32_t*)(a.block + d->cursor);
    int32_t* kfkey = (int32_t*)(a.block + d->kfkey);
    unsigned long long* pairs = (unsigned long long*)(a.block + d->pairs);
    for (int kk = wave; kk < MP_KF_PER_GROUP; kk += MP_WAVES) {
        const int k = k0 + kk;
        if (k >= K) break;
        const LmKeyframeDev* __restrict__ kf = d->kfs + k;
        const int32_t* __restrict__ ob = d->obs + kf->slot_off;
        const bool outside = kfwin[k] < 0;                  // (COUNT: only the local keyframes are numbered yet)
        for (int s = lane; s < kf->n_slots; s += 64) {
            const int p = ob[s];
            if (p < 0) continue;
            const int h = mp_find(table, d->T_bits, p);
            if (h < 0) continue;
            const int lp = cell_lp[h];
            if (lp < 0) continue;
            if (!FILL) {
                atomicAdd(&count[lp], 1);
                if (outside) atomicMin(&kfkey[k], lp);
            } else {                                        // (usable: every segment lies below observation_capacity)
                const int j = off[lp] + atomicAdd(&cursor[lp], 1);
                if (j < off[lp + 1] && j < d->ocap) pairs[j] = ((unsigned long long)(unsigned)k << 32) | (unsigned)s;
            }
        }
    }
}

__device__ __forceinline__ void mp_copy_pose(const MpWinDev* d, int wk, int k, int constant) {
    d->kf_index[wk] = k;
    d->kf_constant[wk] = (uint8_t)constant;
#pragma unroll
    for (int i = 0; i < 12; ++i) d->T_c2w[12 * (size_t)wk + i] = d->kfs[k].T[i];
}

__global__ __launch_bounds__(MP_THREADS) void mapping_win_offsets_kernel(const MpWinArgs a) {
    __shared__ int wsum[MP_WAVES];
    __shared__ int s_fixed;
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.x;
    dsdtm_mapping_window_result* res = (dsdtm_mapping_window_result*)(a.block + d->result);
    const int tid = threadIdx.x, K = d->K, n_local = d->n_local, n_points = res->n_points;
    const int32_t* __restrict__ local = (const int32_t*)(a.block + d->local);
    const int32_t* __restrict__ kfkey = (const int32_t*)(a.block + d->kfkey);
    const int32_t* __restrict__ count = (const int32_t*)(a.block + d->count);
    int32_t* kfwin = (int32_t*)(a.block + d->kfwin);
    int32_t* off = (int32_t*)(a.block + d->off);
    if (tid == 0) s_fixed = 0;
    __syncthreads();
    int origin_local = 0;
    for (int r = 0; r < n_local; ++r) origin_local |= local[r] == d->origin ? 1 : 0;
    for (int r = tid; r < n_local; r += MP_THREADS)
        if (r < d->kcap) mp_copy_pose(d, r, local[r], local[r] == d->origin ? 1 : 0);
    int fixed = 0;
    for (int k = tid; k < K; k += MP_THREADS) {
        const int key = kfkey[k];
        if (key == MP_NONE) continue;
        ++fixed;
        int rank = 0;                                       // first occurrence: ascending (first window point observed, keyframe)
        for (int q = 0; q < K; ++q) {
            const int kq = kfkey[q];
            rank += (kq < key || (kq == key && q < k)) ? 1 : 0;      // (MP_NONE is the largest int: never below a key)
        }
        const int wk = n_local + rank;
        if (wk < d->kcap) { kfwin[k] = wk; mp_copy_pose(d, wk, k, 1); }
    }
    if (fixed) atomicAdd(&s_fixed, fixed);
    int run = 0;
    for (int base = 0; base < n_points; base += MP_THREADS) {
        const int lp = base + tid;
        const int c = lp < n_points ? count[lp] : 0;
        int total;
        const int at = run + mp_scan(c, wsum, total);
        if (lp < n_points) off[lp] = at;
        run += total;
    }
    __syncthreads();
    if (tid == 0) {
        off[n_points] = run;
        const int n_fixed = s_fixed, n_free = n_local - origin_local, n_const = n_fixed + origin_local;
        dsdtm_mapping_window_result r;
        r.n_local = n_local; r.n_fixed = n_fixed; r.n_points = n_points; r.n_obs = run;
        r.over_free_kf = n_free > DSDTM_LBA_MAX_FREE_KF; r.over_const_kf = n_const > DSDTM_LBA_MAX_CONST_KF;
        r.over_points = n_points > DSDTM_LBA_MAX_POINTS; r.over_obs = run > DSDTM_LBA_MAX_OBSERVATIONS;
        r.over_keyframe_capacity = n_local + n_fixed > d->kcap; r.over_point_capacity = n_points > d->pcap;
        r.over_observation_capacity = run > d->ocap;
        r.usable = (n_free >= 1 && !(r.over_free_kf | r.over_const_kf | r.over_points | r.over_obs | r.over_keyframe_capacity |
                                     r.over_point_capacity | r.over_observation_capacity)) ? 1 : 0;
        *res = r;
    }
}

__global__ __launch_bounds__(MP_THREADS) void mapping_win_emit_kernel(const MpWinArgs a) {
    const MpWinDev* d = (const MpWinDev*)a.block + blockIdx.y;
    const dsdtm_mapping_window_result* res = (const dsdtm_mapping_window_result*)(a.block + d->result);
    const int j = (int)blockIdx.x * MP_THREADS + (int)threadIdx.x;
    if (!res->usable || j >= res->n_obs || j >= d->ocap) return;
    const int32_t* __restrict__ off = (const int32_t*)(a.block + d->off);
    const int32_t* __restrict__ kfwin = (const int32_t*)(a.block + d->kfwin);
    int lo = 0, hi = res->n_points;                         // the last point whose offset is <= j: the segment j lies in
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    const int s0 = off[lo], s1 = off[lo + 1];
    const unsigned long long* __restrict__ pairs = (const unsigned long long*)(a.block + d->pairs);
    const unsigned long long me = pairs[j];
    int rank = 0;
    for (int q = s0; q < s1; ++q) rank += pairs[q] < me ? 1 : 0;
    const int o = s0 + rank, k = (int)(me >> 32), s = (int)(me & 0xffffffffull);
    if ((unsigned)k >= (unsigned)d->K || (unsigned)s >= (unsigned)d->kfs[k].n_slots) return;      // (keys are (keyframe, slot) pairs of the map)
    const TmFeatDev f = d->feat[d->kfs[k].slot_off + s];
    d->obs_kf[o] = kfwin[k];
    d->obs_point[o] = lo;
    d->obs_level[o] = f.level;
    d->obs_bearing[3 * (size_t)o] = f.bearing[0]; d->obs_bearing[3 * (size_t)o + 1] = f.bearing[1]; d->obs_bearing[3 * (size_t)o + 2] = f.bearing[2];
    d->obs_slot[o] = (int64_t)me;
}

// ---------------------------------------------------------------------------------------------------------------------- commit

__global__ __launch_bounds__(MP_THREADS) void mapping_fill_kernel(int32_t* dst, unsigned long long words, int32_t value) {
    const unsigned long long i = (unsigned long long)blockIdx.x * MP_THREADS + threadIdx.x;
    if (i < words) dst[i] = value;
}

template <bool VERIFY>
__global__ __launch_bounds__(MP_THREADS) void mapping_commit_claim_kernel(const MpCommitArgs a) {
    const MpCommitDev* d = (const MpCommitDev*)a.block + blockIdx.y;
    const int i = (int)blockIdx.x * MP_THREADS + (int)threadIdx.x;
    int32_t* claim_k = (int32_t*)(a.block + d->claim_k);
    int32_t* claim_p = (int32_t*)(a.block + d->claim_p);
    unsigned long long* verdict = (unsigned long long*)(a.block + a.verdict);
    int32_t* cell[2] = {nullptr, nullptr};
    if (i < d->n_kf && (unsigned)d->kf_index[i] < (unsigned)d->K) cell[0] = claim_k + d->kf_index[i];
    if (i < d->n_points && (unsigned)d->point_index[i] < (unsigned)d->P) cell[1] = claim_p + d->point_index[i];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!cell[c]) continue;
        if (!VERIFY) atomicMin(cell[c], d->window);
        else if (*cell[c] != d->window) atomicMin(verdict, ((unsigned long long)(unsigned)*cell[c] << 32) | (unsigned)d->window);
    }
}

__global__ __launch_bounds__(MP_THREADS) void mapping_commit_apply_kernel(const MpCommitArgs a) {
    const MpCommitDev* d = (const MpCommitDev*)a.block + blockIdx.y;
    const int i = (int)blockIdx.x * MP_THREADS + (int)threadIdx.x;
    if (i < d->n_kf) {                                      // C1: every window keyframe's pose, constant ones included
        const int k = d->kf_index[i];
        if ((unsigned)k < (unsigned)d->K)
#pragma unroll
            for (int e = 0; e < 12; ++e) d->kfs[k].T[e] = d->T_c2w[12 * (size_t)i + e];
    }
    if (i >= d->n_points) return;
    int32_t* went_bad = (int32_t*)(a.block + d->went_bad);
    int32_t* n_out = (int32_t*)(a.block + d->n_out);
    went_bad[i] = 0; n_out[i] = 0;
    const int p = d->point_index[i];
    if ((unsigned)p >= (unsigned)d->P) return;
    d->points[p].x = d->pts[3 * (size_t)i]; d->points[p].y = d->pts[3 * (size_t)i + 1]; d->points[p].z = d->pts[3 * (size_t)i + 2];
    // C2: the point's observations are [b0, b1) (obs_point does not decrease)
    int b[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        int lo = 0, hi = d->n_obs;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (d->obs_point[mid] < i + c) lo = mid + 1; else hi = mid;
        }
        b[c] = lo;
    }
    const int n0 = b[1] - b[0];
    int outliers = 0, erased = 0, bad = 0;                  // erased: the outliers taken while the point was good (their slots are kept)
    for (int j = b[0]; j < b[1]; ++j) {
        if (!d->outlier[j]) continue;
        ++outliers;
        if (bad) continue;                                  // (Erase_Observation finds nothing: the observations are gone)
        ++erased;
        if (n0 - erased <= 1) bad = 1;
    }
    int seen = 0;
    for (int j = b[0]; j < b[1]; ++j) {
        const unsigned long long key = (unsigned long long)d->obs_slot[j];
        const int k = (int)(key >> 32), s = (int)(key & 0xffffffffull);
        if ((unsigned)k >= (unsigned)d->K || (unsigned)s >= (unsigned)d->kfs[k].n_slots) continue;
        const int64_t at = d->kfs[k].slot_off + s;
        if (d->outlier[j] && seen < erased) {               // the j-th outlier: observes cleared, point_of_slot KEPT
            ++seen;
            d->obs[at] = -1;
        } else if (bad) {                                   // SetBadFlag: what is still left
            d->obs[at] = -1;
            d->slots[at] = -1;
        }
    }
    if (bad) d->points[p].bad = 1ull;
    went_bad[i] = bad; n_out[i] = outliers;
}

__global__ __launch_bounds__(MP_THREADS) void mapping_commit_collect_kernel(const MpCommitArgs a) {
    __shared__ int wsum[MP_WAVES];
    const MpCommitDev* d = (const MpCommitDev*)a.block + blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t* __restrict__ went_bad = (const int32_t*)(a.block + d->went_bad);
    const int32_t* __restrict__ n_out = (const int32_t*)(a.block + d->n_out);
    int32_t* bad_list = (int32_t*)(a.block + d->bad_list);
    int run = 0, outliers = 0;
    for (int base = 0; base < d->n_points; base += MP_THREADS) {
        const int i = base + tid;
        const int flag = i < d->n_points ? went_bad[i] : 0;
        int total, total_out;
        const int at = run + mp_scan(flag, wsum, total);
        (void)mp_scan(i < d->n_points ? n_out[i] : 0, wsum, total_out);
        if (flag && at < d->bad_cap) bad_list[at] = d->point_index[i];
        run += total; outliers += total_out;
    }
    if (tid == 0) {
        dsdtm_mapping_commit_result r;
        r.n_outliers = outliers; r.n_bad = run; r.overflow_bad = run > d->bad_cap ? 1 : 0; r.reserved = 0;
        *(dsdtm_mapping_commit_result*)(a.block + d->result) = r;
    }
}

}  // namespace

#define MP_LAUNCH(kernel, grid, ...)                                                          \
    do {                                                                                      \
        hipLaunchKernelGGL(kernel, grid, dim3(MP_THREADS), 0, stream, __VA_ARGS__);           \
        if (hipError_t e_ = hipGetLastError()) return e_;                                     \
    } while (0)

hipError_t mapping_covisibility_launch(const MpCovArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)args.n;
    if (args.max_K > 0) MP_LAUNCH(mapping_cov_weight_kernel, dim3(mp_groups(args.max_K, MP_KF_PER_GROUP), n), args);
    MP_LAUNCH(mapping_cov_list_kernel, dim3(n), args);
    return hipSuccess;
}

hipError_t mapping_window_launch(const MpWinArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)args.n;
    const long long widest = args.max_T > args.max_K ? (args.max_T > args.max_E ? args.max_T : args.max_E) : (args.max_K > args.max_E ? args.max_K : args.max_E);
    MP_LAUNCH(mapping_win_init_kernel, dim3(mp_groups(widest, MP_THREADS), n), args);
    MP_LAUNCH(mapping_win_insert_kernel, dim3(mp_groups(args.max_E > MP_THREADS ? args.max_E : MP_THREADS, MP_THREADS), n), args);
    MP_LAUNCH(mapping_win_first_kernel, dim3(n), args);
    MP_LAUNCH(mapping_win_scan_kernel<false>, dim3(mp_groups(args.max_K, MP_KF_PER_GROUP), n), args);
    MP_LAUNCH(mapping_win_offsets_kernel, dim3(n), args);
    if (args.max_ocap > 0) {
        MP_LAUNCH(mapping_win_scan_kernel<true>, dim3(mp_groups(args.max_K, MP_KF_PER_GROUP), n), args);
        MP_LAUNCH(mapping_win_emit_kernel, dim3(mp_groups(args.max_ocap, MP_THREADS), n), args);
    }
    return hipSuccess;
}

hipError_t mapping_commit_check_launch(const MpCommitArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)args.n;
    MP_LAUNCH(mapping_fill_kernel, dim3(mp_groups((long long)args.claim_words, MP_THREADS)), (int32_t*)(args.block + args.verdict),
              (unsigned long long)args.claim_words, (int32_t)MP_NONE);
    MP_LAUNCH(mapping_commit_claim_kernel<false>, dim3(mp_groups(args.max_items, MP_THREADS), n), args);
    MP_LAUNCH(mapping_commit_claim_kernel<true>, dim3(mp_groups(args.max_items, MP_THREADS), n), args);
    return hipSuccess;
}

hipError_t mapping_commit_apply_launch(const MpCommitArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)args.n;
    MP_LAUNCH(mapping_commit_apply_kernel, dim3(mp_groups(args.max_items, MP_THREADS), n), args);
    MP_LAUNCH(mapping_commit_collect_kernel, dim3(n), args);
    return hipSuccess;
}

}  // namespace dsdtm
