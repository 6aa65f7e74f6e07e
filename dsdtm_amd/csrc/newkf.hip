// newkf.hip — the kernel of libdsdtm_amd_newkf.so (include/dsdtm_amd_newkf.h): what Tracking::CraeteKeyframe (src/Tracking.cpp:412-464)
// does between the per-cell corners of Feature_detector::detect and the keyframe's slots, for n trackers, ONE 256-thread workgroup per
// tracker. Rules K1-K6 are the header's. In order:
//   candidates   the cells above the floor whose pixel is inside the image become keys (~score bits, cell index) in LDS (K2); a
//                bitonic network orders them: ascending keys = descending score, equal scores by cell index.
//   K3           one thread per candidate: the discs of the existing features that have a point (half-width table per |dy|) and the
//                dynamic mask; a masked candidate is flagged in its pixel word.
//   K4           the sequential recurrence: wavefront 0 walks the candidates in order. The accepted corners lie in square bins of
//                side >= cell_size (lists in LDS), so a candidate meets only the nine bins around it, one lane per bin, and a ballot
//                decides. The accepted list is compacted IN PLACE over the candidates already walked (accepted <= walked), so
//                candidates and accepted share 48 KB of LDS; the bins' heads take 8 KB more.
//   K5, K6       one thread per slot, 256 slots per trip: the feature columns, the lift (the formulas of rgbd.hip's lift_kernel on the
//                caller's u16 depth: d * (1.0f / depth_scale) is what depth_ingest_kernel keeps), and a ballot prefix sum over the
//                slots that numbers the new points.
// Integer logic, copies and the double-precision formulas that rgbd.hip and track.hip evaluate bit-equal to their restatements;
// floating-point contraction is off. Plain C++ and wave intrinsics only.
#include "newkf.h"

namespace dsdtm {

#define NEWKF_THREADS 256
#define NEWKF_MASKED 0x80000000u
#define NEWKF_BINS 64                                  // K4's bins: at most 64 x 64 over the image
#define NEWKF_NONE 0xffffu

struct NewkfLds {
    unsigned long long keys[DSDTM_NEWKF_MAX_CELLS];    // candidates in K2's order; [0, n_acc) the accepted ones once K4 has passed them
    unsigned xy[DSDTM_NEWKF_MAX_CELLS];                // x | y << 16 | NEWKF_MASKED, beside keys
    unsigned short head[NEWKF_BINS * NEWKF_BINS];      // K4: the last accepted corner of every bin, NEWKF_NONE = empty
    unsigned char hw_min[128], hw_cell[128];
    int n_cand, n_acc;
    int wsum[NEWKF_THREADS / 64];
};

// cvRound of a float: to nearest, halves to even (saturates; the host refused what is not finite)
__device__ __forceinline__ int newkf_round(float v) { return __float2int_rn(v); }

// Frame::Get_FeatureDetph(cv::Point2f) (src/Frame.cpp:201-224) on the u16 image: -1 when the pixel and its four neighbours hold none
__device__ __forceinline__ float newkf_depth(const NewkfTrackerDev& t, int w, int h, float px, float py) {
    const int x = newkf_round(px), y = newkf_round(py);
    float d = -1.0f;
    if (x >= 0 && x < w && y >= 0 && y < h) {
        const float c = (float)t.depth[(size_t)y * t.depth_stride + x] * t.inv_depth_scale;
        if (c != 0.0f) d = c;
        else {
            const int dx[4] = {-1, 0, 1, 0}, dy[4] = {0, -1, 0, 1};
            bool found = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x + dx[k], yy = y + dy[k];
                if (found || xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                const float v = (float)t.depth[(size_t)yy * t.depth_stride + xx] * t.inv_depth_scale;
                if (v != 0.0f) { d = v; found = true; }
            }
        }
    }
    return d;
}

__global__ __launch_bounds__(NEWKF_THREADS) void newkf_make_kernel(const NewkfArgs a) {
#pragma clang fp contract(off)
    __shared__ NewkfLds L;
    const NewkfTrackerDev t = a.trackers[blockIdx.x];         // (uniform: a copy in scalar registers)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.prm.width, H = a.prm.height, G = a.prm.grid_cols * a.prm.grid_rows;
    const int ne = t.n_existing;
    if (tid < 128) { L.hw_min[tid] = a.hw_min[tid]; L.hw_cell[tid] = a.hw_cell[tid]; }
    if (tid == 0) { L.n_cand = 0; L.n_acc = 0; }
    for (int i = tid; i < NEWKF_BINS * NEWKF_BINS; i += NEWKF_THREADS) L.head[i] = NEWKF_NONE;
    __syncthreads();

    if (ne < a.prm.max_fts) {                                       // K1
        // ---- K2: the candidates and their order
        for (int k = tid; k < G; k += NEWKF_THREADS) {
            const float s = t.cell_score[k];
            if (!(s > a.prm.score_floor)) continue;                 // (a NaN never passes)
            const int x = t.cell_x[k], y = t.cell_y[k], l = t.cell_level[k];
            if (x < 0 || x >= W || y < 0 || y >= H || l < 0 || l > 15) continue;
            const int pos = atomicAdd(&L.n_cand, 1);                // (any order: the keys are distinct and sorted next)
            L.keys[pos] = ((unsigned long long)(~__float_as_uint(s)) << 32) | (unsigned)k;
        }
        __syncthreads();
        const int nc = L.n_cand;
        int P = 1;
        while (P < nc) P <<= 1;
        for (int i = nc + tid; i < P; i += NEWKF_THREADS) L.keys[i] = ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += NEWKF_THREADS) {
                    const int o = i ^ j;
                    if (o > i) {
                        const unsigned long long u = L.keys[i], v = L.keys[o];
                        if ((u > v) == ((i & k) == 0)) { L.keys[i] = v; L.keys[o] = u; }
                    }
                }
                __syncthreads();
            }
        // ---- K3: the mask Set_Mask would have painted, read at every candidate's pixel
        const int rmin = a.prm.min_dist;
        for (int i = tid; i < nc; i += NEWKF_THREADS) {
            const int k = (int)(L.keys[i] & 0xffffu);
            const int x = t.cell_x[k], y = t.cell_y[k];
            bool masked = false;
            if (ne > 0) {
                for (int e = 0; e < ne && !masked; ++e) {
                    if (!t.has_point[e]) continue;
                    const long long dy = llabs((long long)y - (long long)newkf_round(t.px_xy[2 * e + 1]));
                    if (dy > rmin) continue;
                    const long long dx = llabs((long long)x - (long long)newkf_round(t.px_xy[2 * e]));
                    masked = dx <= (long long)L.hw_min[dy];
                }
                if (!masked && t.dyn) masked = t.dyn[(size_t)y * t.dyn_stride + x] > 200;
            }
            L.xy[i] = (unsigned)x | ((unsigned)y << 16) | (masked ? NEWKF_MASKED : 0u);
        }
        __syncthreads();
        // ---- K4: the walk. An accepted corner can only cover a later one that lies within cell_size of it in x and in y, so the
        // accepted corners are kept in square bins of side B >= cell_size (B also large enough that 64 x 64 bins cover the image),
        // each bin a list through the high words of keys[] (the score bits are spent once the order is made): a candidate looks
        // into its own bin and the eight around it, one lane per bin, and a ballot decides.
        if (wave == 0) {
            const int room = a.prm.max_fts - ne, rc = a.prm.cell_size;
            int B = rc > 1 ? rc : 1;
            B = max(B, max((W + NEWKF_BINS - 1) / NEWKF_BINS, (H + NEWKF_BINS - 1) / NEWKF_BINS));
            const int nbx = (W + B - 1) / B, nby = (H + B - 1) / B;            // <= NEWKF_BINS each
            int nacc = 0;
            for (int i = 0; i < nc; ++i) {
                const unsigned c = L.xy[i];
                if (c & NEWKF_MASKED) continue;
                const int x = (int)(c & 0xffffu), y = (int)(c >> 16);
                const int bx = x / B, by = y / B;
                bool hit = false;
                if (lane < 9) {
                    const int qx = bx + lane % 3 - 1, qy = by + lane / 3 - 1;
                    if (qx >= 0 && qx < nbx && qy >= 0 && qy < nby) {
                        unsigned j = L.head[qy * nbx + qx];
                        while (j != NEWKF_NONE && !hit) {
                            const unsigned v = L.xy[j];
                            const unsigned nxt = (unsigned)(L.keys[j] >> 32);
                            const int dy = abs(y - (int)(v >> 16)), dx = abs(x - (int)(v & 0xffffu));
                            if (dy <= rc && dx <= rc) hit = dx <= (int)L.hw_cell[dy];
                            j = nxt;
                        }
                    }
                }
                if (__ballot(hit) != 0ull) continue;
                // (every lane stores the same words: each lane's later reads follow its own store)
                const unsigned cell = (unsigned)(L.keys[i] & 0xffffu);
                const unsigned prev = L.head[by * nbx + bx];
                L.xy[nacc] = c; L.keys[nacc] = ((unsigned long long)prev << 32) | cell;
                L.head[by * nbx + bx] = (unsigned short)nacc;
                nacc++;
                if (nacc >= room) break;
            }
            if (lane == 0) L.n_acc = nacc;
        }
        __syncthreads();
    }

    // ---- K5 + K6: the slots
    const int n_new = L.n_acc, n_slots = ne + n_new;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run = 0;                                                    // new points in the slots before this trip
    for (int base = 0; base < n_slots; base += NEWKF_THREADS) {
        const int i = base + tid;
        float px = 0.0f, py = 0.0f, dep = -1.0f;
        int lvl = 0, pos = -1;
        double b0 = 0.0, b1 = 0.0, b2 = 0.0, pw[3] = {0.0, 0.0, 0.0};
        bool lift = false, made = false;
        if (i < n_slots) {
            if (i < ne) {
                px = t.px_xy[2 * i]; py = t.px_xy[2 * i + 1]; lvl = t.level[i];
                b0 = t.bearing[3 * i]; b1 = t.bearing[3 * i + 1]; b2 = t.bearing[3 * i + 2];
                if (t.initial[i]) pos = t.point_index[i];           // :428-433
                else lift = true;
            } else {
                const unsigned c = L.xy[i - ne];
                px = (float)(int)(c & 0xffffu); py = (float)(int)(c >> 16);
                lvl = t.cell_level[(int)(L.keys[i - ne] & 0xffffu)];
                // Frame::Add_Feature: mNormal = Pixel2Camera(cv::Point2f, 1.0f) in float, normalised in double (as track.hip)
                const float one = 1.0f;
                const double bx = (double)((one * (px - a.cx)) / a.fx), by = (double)((one * (py - a.cy)) / a.fy);
                const double nrm = sqrt(bx * bx + by * by + 1.0 * 1.0);
                b0 = bx / nrm; b1 = by / nrm; b2 = 1.0 / nrm;
                lift = true;
            }
            if (lift) {
                dep = newkf_depth(t, W, H, px, py);
                if (!(dep < 0.0f)) {                                // :437 z < 0: no point
                    made = true;
                    // Frame::UnProject: Pixel2Camera in float, then mT_c2w.inverse() * p as Sophus: R^T p + (-(R^T t))
                    const float cxf = dep * (px - a.cx) / a.fx, cyf = dep * (py - a.cy) / a.fy;
                    const double p0 = (double)cxf, p1 = (double)cyf, p2 = (double)dep;
                    const double* T = t.T;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double rp = T[c] * p0 + T[4 + c] * p1 + T[8 + c] * p2;
                        const double rt = T[c] * T[3] + T[4 + c] * T[7] + T[8 + c] * T[11];
                        pw[c] = rp + (-rt);
                    }
                }
            }
        }
        const unsigned long long m = __ballot(made);
        if (lane == 0) L.wsum[wave] = __popcll(m);
        __syncthreads();
        int rank = run + __popcll(m & below), total = 0;
        for (int w = 0; w < NEWKF_THREADS / 64; ++w) { if (w < wave) rank += L.wsum[w]; total += L.wsum[w]; }
        __syncthreads();
        run += total;
        if (made) {
            pos = t.first_point_index + rank;
            if (rank < t.out_points) { t.o_p_world[3 * (size_t)rank] = pw[0]; t.o_p_world[3 * (size_t)rank + 1] = pw[1]; t.o_p_world[3 * (size_t)rank + 2] = pw[2]; }
        }
        if (i < n_slots && i < t.out_slots) {
            t.o_point_of_slot[i] = pos; t.o_observes[i] = pos >= 0 ? 1 : 0;
            t.o_px_xy[2 * (size_t)i] = px; t.o_px_xy[2 * (size_t)i + 1] = py; t.o_level[i] = lvl;
            t.o_bearing[3 * (size_t)i] = b0; t.o_bearing[3 * (size_t)i + 1] = b1; t.o_bearing[3 * (size_t)i + 2] = b2;
            t.o_depth[i] = dep;
        }
    }
    if (tid == 0) {
        t.counts[0] = n_new; t.counts[1] = n_slots; t.counts[2] = run;
        t.counts[3] = (n_slots > t.slot_cap || run > t.point_cap || (t.bad_cap >= 0 && run > t.bad_cap)) ? 1 : 0;
    }
}

hipError_t newkf_make_launch(const NewkfArgs& args, hipStream_t stream) {
    if (!args.trackers || args.n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(newkf_make_kernel, dim3((unsigned)args.n), dim3(NEWKF_THREADS), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
