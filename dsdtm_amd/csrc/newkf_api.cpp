// newkf_api.cpp — the C ABI of include/dsdtm_amd_newkf.h (libdsdtm_amd_newkf.so): checks, staging, launch (the context: addon_host.h).
//
// dsdtm_newkf_make_batch checks every tracker, lays ONE block out (the trackers' records, their existing-feature columns, every
// caller array that has to be staged, then the results), fills the pinned side, moves the front with a single hipMemcpyAsync, launches
// newkf.hip's kernel, copies the results back and waits once. There is no CPU compute path here (the host evaluation of the same
// rules is create_keyframe_host of host/dsdtm_newkf_host.hpp, which needs no library).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "newkf.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_newkf_ctx : dsdtm::AddonCtx {};      // (staging: the upload and the results, at the same offsets on both sides)

extern "C" const char* dsdtm_newkf_last_error(const dsdtm_newkf_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_newkf_create(int device, dsdtm_newkf_ctx** out) { return addon_create("dsdtm_amd_newkf", device, out); }
extern "C" void dsdtm_newkf_destroy(dsdtm_newkf_ctx* ctx) { addon_destroy(ctx); }

// dy -> half-width of cv::circle(.., radius, .., -1) (OpenCV drawing.cpp Circle(), filled): the midpoint walk, each step giving the rows
// +-dy the half-width dx and the rows +-dx the half-width dy; a row keeps its widest span. 0 <= radius <= 127.
static void span_table(int radius, uint8_t hw[128]) {
    memset(hw, 0, 128);
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = (uint8_t)std::max<int>(hw[dy], dx);
        hw[dx] = (uint8_t)std::max<int>(hw[dx], dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// ---- where a caller's image-like array lives, and how the kernel gets at it: THE rule for the cells, the depth image and the dynamic mask
enum { MEM_PAGEABLE = 0, MEM_PINNED = 1, MEM_DEVICE = 2, MEM_OTHER_DEVICE = -1 };
struct CallerArray {
    const void* p = nullptr;
    size_t row_bytes = 0, rows = 0, pitch = 0;     // pitch in bytes (the caller's); a staged copy is packed: pitch = row_bytes
    int mem = MEM_PAGEABLE;
    size_t off = 0;                                // MEM_PAGEABLE: where in the block
};
// the kind is found once per pointer
static int array_memory(const dsdtm_newkf_ctx* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return MEM_PAGEABLE; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? MEM_DEVICE : MEM_OTHER_DEVICE;
    if (pa_.type == hipMemoryTypeHost) return MEM_PINNED;
    return MEM_PAGEABLE;
}
// a pageable array takes row_bytes * rows of the block at *cursor
static CallerArray caller_array(const dsdtm_newkf_ctx* ctx, const void* p, size_t row_bytes, size_t rows, size_t pitch, size_t* cursor) {
    CallerArray a;
    a.p = p; a.row_bytes = row_bytes; a.rows = rows; a.pitch = pitch;
    a.mem = array_memory(ctx, p);
    if (a.mem == MEM_PAGEABLE) { a.off = *cursor; *cursor = align_up(*cursor + row_bytes * rows, 16); }
    return a;
}
// the device address and the pitch the kernel reads it with; a pageable array is copied into the pinned block here
static int place_array(dsdtm_newkf_ctx* ctx, const CallerArray& a, const void** dev, size_t* pitch) {
    *pitch = a.pitch;
    if (a.mem == MEM_DEVICE) { *dev = a.p; return DSDTM_OK; }
    if (a.mem == MEM_PINNED) {
        void* d = nullptr;
        HIP_TRY(ctx, hipHostGetDevicePointer(&d, const_cast<void*>(a.p), 0));
        *dev = d;
        return DSDTM_OK;
    }
    uint8_t* h = (uint8_t*)ctx->h_pinned + a.off;
    for (size_t r = 0; r < a.rows; ++r) memcpy(h + r * a.row_bytes, (const uint8_t*)a.p + r * a.pitch, a.row_bytes);
    *dev = (const uint8_t*)ctx->d_stage + a.off;
    *pitch = a.row_bytes;
    return DSDTM_OK;
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

struct TrackerPlan {
    CallerArray cell[4], depth, dyn;
    size_t in_px, in_level, in_bearing, in_has, in_initial, in_point;      // the existing-feature columns in the block
    size_t out_counts, out_pos, out_obs, out_px, out_level, out_bearing, out_depth, out_pw;
    int out_slots, out_points;
};

extern "C" int dsdtm_newkf_make_batch(dsdtm_newkf_ctx* ctx, const dsdtm_camera* cam, const dsdtm_newkf_params* prm, int n,
                                      const dsdtm_newkf_desc* descs, dsdtm_newkf_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam) { set_err(ctx, "newkf_make: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!prm) { set_err(ctx, "newkf_make: params is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 1 || n > DSDTM_NEWKF_MAX_TRACKERS) { set_err(ctx, "newkf_make: n = %d outside 1..%d", n, DSDTM_NEWKF_MAX_TRACKERS); return DSDTM_ERR_INVALID; }
    if (!descs || !results) { set_err(ctx, "newkf_make: %s is NULL", !descs ? "descs" : "results"); return DSDTM_ERR_INVALID; }
    {
        const char* bad = nullptr;
        if (prm->width < 1 || prm->width > DSDTM_NEWKF_MAX_SIDE) bad = "width";
        else if (prm->height < 1 || prm->height > DSDTM_NEWKF_MAX_SIDE) bad = "height";
        else if (prm->cell_size < 0 || prm->cell_size > DSDTM_NEWKF_MAX_RADIUS) bad = "cell_size";
        else if (prm->min_dist < 0 || prm->min_dist > DSDTM_NEWKF_MAX_RADIUS) bad = "min_dist";
        else if (prm->grid_cols < 1 || prm->grid_rows < 1 || (long long)prm->grid_cols * prm->grid_rows > DSDTM_NEWKF_MAX_CELLS) bad = "grid_cols x grid_rows";
        else if (prm->max_fts < 0) bad = "max_fts";
        else if (!std::isfinite(prm->score_floor) || prm->score_floor < 0.0f) bad = "score_floor";
        if (bad) { set_err(ctx, "newkf_make: params: %s out of range", bad); return DSDTM_ERR_INVALID; }
        if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy) || cam->fx == 0.0f || cam->fy == 0.0f) {
            set_err(ctx, "newkf_make: cam: fx, fy, cx, cy must be finite and fx, fy non-zero");
            return DSDTM_ERR_INVALID;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)n, G = (size_t)prm->grid_cols * (size_t)prm->grid_rows, W = (size_t)prm->width, H = (size_t)prm->height;
    // every tracker is checked before anything is enqueued; the block's layout on the way
    std::vector<TrackerPlan> plan(N);
    size_t o = align_up(N * sizeof(NewkfTrackerDev), 16);
    for (int t = 0; t < n; ++t) {
        const dsdtm_newkf_desc& d = descs[t];
        const dsdtm_newkf_result& r = results[t];
        TrackerPlan& p = plan[(size_t)t];
        const char* bad = nullptr;
        int at = -1;
        const size_t ne = d.n_existing > 0 ? (size_t)d.n_existing : 0;
        if (d.n_existing < 0 || d.n_existing > DSDTM_NEWKF_MAX_EXISTING) bad = "n_existing out of range";
        else if (!d.cell_score || !d.cell_x || !d.cell_y || !d.cell_level) bad = "a cell array is NULL";
        else if (ne && (!d.px_xy || !d.level || !d.bearing || !d.has_point || !d.initial || !d.point_index)) bad = "an existing-feature array is NULL";
        else if (!d.depth) bad = "depth is NULL";
        else if (d.depth_stride < prm->width) bad = "depth_stride below width";
        else if (!(d.depth_scale > 0.0f) || !std::isfinite(d.depth_scale) || !std::isfinite(1.0f / d.depth_scale)) bad = "depth_scale is not a positive finite number";
        else if (d.dyn_mask && d.dyn_stride < prm->width) bad = "dyn_stride below width";
        else if (!d.T_c2w) bad = "T_c2w is NULL";
        else if (!all_finite(d.T_c2w, 12)) bad = "T_c2w is not finite";
        else if (d.first_point_index < 0) bad = "first_point_index is negative";
        else if (d.slot_capacity < d.n_existing) bad = "slot_capacity below n_existing";
        else if (d.point_capacity < 0) bad = "point_capacity is negative";
        else if (r.new_bad && d.bad_capacity < 0) bad = "bad_capacity is negative";
        else if (d.slot_capacity > 0 && (!r.point_of_slot || !r.observes || !r.px_xy || !r.level || !r.bearing || !r.depth_of_slot)) bad = "a slot column of the result is NULL";
        else if (d.point_capacity > 0 && !r.new_p_world) bad = "new_p_world is NULL";
        for (size_t k = 0; !bad && k < ne; ++k) {
            at = (int)k;
            if (!std::isfinite(d.px_xy[2 * k]) || !std::isfinite(d.px_xy[2 * k + 1])) bad = "px_xy is not finite";
            else if (d.level[k] < 0 || d.level[k] > 15) bad = "level outside 0..15";
            else if (d.initial[k] && d.point_index[k] < 0) bad = "initial feature with point_index < 0";
        }
        if (!bad) {
            at = -1;
            p.in_px = o; o = align_up(o + ne * 8, 16);
            p.in_level = o; o = align_up(o + ne * 4, 16);
            p.in_bearing = o; o = align_up(o + ne * 24, 16);
            p.in_has = o; o = align_up(o + ne, 16);
            p.in_initial = o; o = align_up(o + ne, 16);
            p.in_point = o; o = align_up(o + ne * 4, 16);
            const void* cells[4] = {d.cell_score, d.cell_x, d.cell_y, d.cell_level};
            for (int c = 0; c < 4 && !bad; ++c) {
                p.cell[c] = caller_array(ctx, cells[c], G * 4, 1, G * 4, &o);
                if (p.cell[c].mem == MEM_OTHER_DEVICE) bad = "a cell array lies in another device's memory";
            }
            // cells the host can read are checked here; cells in device memory are the kernel's to skip
            for (int c = 1; c < 4 && !bad; ++c) {
                if (p.cell[c].mem == MEM_DEVICE) continue;
                const int32_t* v = (const int32_t*)cells[c];
                for (size_t k = 0; k < G && !bad; ++k)
                    if (v[k] < 0) { at = (int)k; bad = c == 1 ? "cell_x is negative" : c == 2 ? "cell_y is negative" : "cell_level is negative"; }
            }
        }
        if (!bad) {
            p.depth = caller_array(ctx, d.depth, W * 2, H, (size_t)d.depth_stride * 2, &o);
            if (p.depth.mem == MEM_OTHER_DEVICE) bad = "depth lies in another device's memory";
        }
        if (!bad && d.dyn_mask) {
            p.dyn = caller_array(ctx, d.dyn_mask, W, H, (size_t)d.dyn_stride, &o);
            if (p.dyn.mem == MEM_OTHER_DEVICE) bad = "dyn_mask lies in another device's memory";
        }
        if (bad) {
            if (at >= 0) set_err(ctx, "newkf_make: tracker %d: %s (entry %d)", t, bad, at);
            else set_err(ctx, "newkf_make: tracker %d: %s", t, bad);
            return DSDTM_ERR_INVALID;
        }
    }
    const size_t upload = align_up(o, 256);
    // the results behind the upload: no tracker can reach more slots than its existing features plus what the walk can add
    o = upload;
    for (int t = 0; t < n; ++t) {
        const dsdtm_newkf_desc& d = descs[t];
        TrackerPlan& p = plan[(size_t)t];
        const long long room = d.n_existing < prm->max_fts ? std::min<long long>((long long)G, (long long)prm->max_fts - d.n_existing) : 0;
        const long long reach = (long long)d.n_existing + room;
        p.out_slots = (int)std::min<long long>(d.slot_capacity, reach);
        p.out_points = (int)std::min<long long>(d.point_capacity, reach);
        const size_t S = (size_t)p.out_slots, P = (size_t)p.out_points;
        p.out_counts = o; o += 16;
        p.out_pos = o; o = align_up(o + S * 4, 16);
        p.out_obs = o; o = align_up(o + S, 16);
        p.out_px = o; o = align_up(o + S * 8, 16);
        p.out_level = o; o = align_up(o + S * 4, 16);
        p.out_bearing = o; o = align_up(o + S * 24, 16);
        p.out_depth = o; o = align_up(o + S * 4, 16);
        p.out_pw = o; o = align_up(o + P * 24, 16);
    }
    const size_t total = o, back = total - upload;
    if (int rc = ensure_stage(ctx, total, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    NewkfTrackerDev* rec = (NewkfTrackerDev*)h;
    for (int t = 0; t < n; ++t) {
        const dsdtm_newkf_desc& d = descs[t];
        const TrackerPlan& p = plan[(size_t)t];
        const size_t ne = (size_t)d.n_existing;
        NewkfTrackerDev k;
        memset(&k, 0, sizeof k);
        if (ne) {
            memcpy(h + p.in_px, d.px_xy, ne * 8); memcpy(h + p.in_level, d.level, ne * 4); memcpy(h + p.in_bearing, d.bearing, ne * 24);
            memcpy(h + p.in_has, d.has_point, ne); memcpy(h + p.in_initial, d.initial, ne); memcpy(h + p.in_point, d.point_index, ne * 4);
        }
        k.px_xy = (const float*)(g + p.in_px); k.level = (const int32_t*)(g + p.in_level); k.bearing = (const double*)(g + p.in_bearing);
        k.has_point = g + p.in_has; k.initial = g + p.in_initial; k.point_index = (const int32_t*)(g + p.in_point);
        const void* dev = nullptr;
        size_t pitch = 0;
        if (int rc = place_array(ctx, p.cell[0], &dev, &pitch)) return rc;
        k.cell_score = (const float*)dev;
        if (int rc = place_array(ctx, p.cell[1], &dev, &pitch)) return rc;
        k.cell_x = (const int32_t*)dev;
        if (int rc = place_array(ctx, p.cell[2], &dev, &pitch)) return rc;
        k.cell_y = (const int32_t*)dev;
        if (int rc = place_array(ctx, p.cell[3], &dev, &pitch)) return rc;
        k.cell_level = (const int32_t*)dev;
        if (int rc = place_array(ctx, p.depth, &dev, &pitch)) return rc;
        k.depth = (const uint16_t*)dev; k.depth_stride = (int32_t)(pitch / 2);
        if (d.dyn_mask) {
            if (int rc = place_array(ctx, p.dyn, &dev, &pitch)) return rc;
            k.dyn = (const uint8_t*)dev; k.dyn_stride = (int32_t)pitch;
        }
        k.inv_depth_scale = 1.0f / d.depth_scale;
        k.n_existing = d.n_existing; k.first_point_index = d.first_point_index;
        k.slot_cap = d.slot_capacity; k.point_cap = d.point_capacity; k.bad_cap = results[t].new_bad ? d.bad_capacity : -1;
        k.out_slots = p.out_slots; k.out_points = p.out_points;
        memcpy(k.T, d.T_c2w, 96);
        k.counts = (int32_t*)(g + p.out_counts);
        k.o_point_of_slot = (int32_t*)(g + p.out_pos); k.o_observes = g + p.out_obs; k.o_px_xy = (float*)(g + p.out_px);
        k.o_level = (int32_t*)(g + p.out_level); k.o_bearing = (double*)(g + p.out_bearing); k.o_depth = (float*)(g + p.out_depth);
        k.o_p_world = (double*)(g + p.out_pw);
        memcpy(&rec[t], &k, sizeof k);
    }
    NewkfArgs a;
    memset(&a, 0, sizeof a);
    a.trackers = (const NewkfTrackerDev*)g; a.n = n;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.prm = *prm;
    span_table(prm->min_dist, a.hw_min);
    span_table(prm->cell_size, a.hw_cell);
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, upload, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(newkf_make_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + upload, g + upload, back, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const TrackerPlan& p = plan[(size_t)t];
        dsdtm_newkf_result& r = results[t];
        int32_t c[4];
        memcpy(c, h + p.out_counts, 16);
        r.n_new = c[0]; r.n_slots = c[1]; r.n_new_points = c[2]; r.overflow = c[3];
        if (r.overflow) continue;
        const size_t S = (size_t)r.n_slots, P = (size_t)r.n_new_points;
        if (S) {
            memcpy(r.point_of_slot, h + p.out_pos, S * 4); memcpy(r.observes, h + p.out_obs, S); memcpy(r.px_xy, h + p.out_px, S * 8);
            memcpy(r.level, h + p.out_level, S * 4); memcpy(r.bearing, h + p.out_bearing, S * 24); memcpy(r.depth_of_slot, h + p.out_depth, S * 4);
        }
        if (P) {
            memcpy(r.new_p_world, h + p.out_pw, P * 24);
            if (r.new_bad) memset(r.new_bad, 0, P);
        }
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_newkf_make(dsdtm_newkf_ctx* ctx, const dsdtm_camera* cam, const dsdtm_newkf_params* prm, const dsdtm_newkf_desc* desc,
                                dsdtm_newkf_result* result) {
    return dsdtm_newkf_make_batch(ctx, cam, prm, 1, desc, result);
}
