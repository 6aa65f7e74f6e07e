// api_track.cpp — dsdtm_track_frame / dsdtm_track_frame_on / dsdtm_track_frames of include/dsdtm_amd.h: one tracked frame, or n of
// them, in one submission (track.hip and the kernels of Run, FindMatchDirect and PoseOptimization). Calls api.cpp for Run
// (launch_batch), the image intake (route_image, enqueue_level0), frame_alloc, the frame pool and the staging blocks.
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "api_internal.h"

using namespace dsdtm;
using namespace dsdtm::detail;

// ---- the checks of a tracked frame's descriptor ------------------------------------------------------
// The checks of a tracked frame's descriptor (dsdtm_track_frame, and every frame of dsdtm_track_frames): nothing is enqueued
// or allocated before they pass.
struct TrackPlan {
    PackedPyr pl;
    int st[DSDTM_MAX_LEVELS];
    int nnz, max_search_level, grid_rows, grid_cols;
    unsigned long long frames_seq;   // the latest prefetch number among the reference frame and the keyframes (frames_consume)
};
// resident: the descriptor of dsdtm_track_frame_on — the new frame is already on the device and `image` must be NULL
static int track_check_desc(dsdtm_ctx* ctx, const dsdtm_camera* cam, const dsdtm_track_desc* d, TrackPlan* out, bool resident = false) {
    if (resident && d->image) { set_err(ctx, "track_frame_on: desc->image must be NULL (the frame is already on the device)"); return DSDTM_ERR_INVALID; }
    if ((!resident && (!d->image || d->stride < d->width)) || d->width <= 0 || d->height <= 0 || d->levels <= 0 || d->levels > DSDTM_MAX_LEVELS ||
        d->width > 16384 || d->height > 16384) { set_err(ctx, "track: bad image geometry"); return DSDTM_ERR_INVALID; }
    // the grid, the packed mask (stride d->width) and the pyramid are sized by the image, the reprojection is bounded by the
    // camera: a camera of another size would read the mask out of bounds (larger) or drop points silently (smaller)
    if (cam->width != d->width || cam->height != d->height) {
        set_err(ctx, "track: camera %dx%d does not match the image %dx%d", cam->width, cam->height, d->width, d->height); return DSDTM_ERR_INVALID;
    }
    if (!d->ref || !d->T_ref_w || !d->T_seed || d->n_ref_features < 0 ||
        (d->n_ref_features > 0 && (!d->ref_px_xy || !d->ref_bearing || !d->ref_p_world || !d->ref_initial))) {
        set_err(ctx, "track: NULL reference-frame argument"); return DSDTM_ERR_INVALID;
    }
    if (d->n_kf < 0 || d->n_kf > 4096 || d->n_points < 0 || d->n_points > 4096 || (d->n_kf > 0 && (!d->kf || !d->T_kf_w)) ||
        (d->n_points > 0 && (!d->mp_world || !d->mp_found || !d->mp_bad || !d->obs_offset))) {
        set_err(ctx, "track: bad local map (at most 4096 keyframes and 4096 map points per call)"); return DSDTM_ERR_INVALID;
    }
    if (d->cell_size <= 0 || d->cell_size > 127 || d->max_matches <= 0 || d->max_matches > 256 || d->align2d_iters < 0 ||
        d->pose_opt.max_iterations < 0 || (d->mask && d->mask_stride < d->width)) {
        set_err(ctx, "track: bad search parameters (cell_size 1..127, max_matches 1..256)"); return DSDTM_ERR_INVALID;
    }
    const int max_search_level = d->max_pyr_levels - 3;                                      // src/Feature_alignment.cpp:144
    if (max_search_level < 0 || max_search_level >= d->levels) { set_err(ctx, "track: max_pyr_levels - 3 outside the pyramid"); return DSDTM_ERR_INVALID; }
    // the new frame's geometry (Frame::ComputeImagePyramid) must be the reference frame's and the keyframes'
    PackedPyr& pl = out->pl;
    plan_image_pyramid(d->width, d->height, d->levels, &pl, out->st);
    auto same_geometry = [&](const dsdtm_frame* f) {
        return f && f->owner == ctx && f->pl.levels == pl.levels && !memcmp(f->pl.w, pl.w, sizeof(int) * pl.levels) &&
               !memcmp(f->pl.h, pl.h, sizeof(int) * pl.levels);
    };
    if (!same_geometry(d->ref)) { set_err(ctx, "track: the reference frame is NULL, foreign or of another geometry"); return DSDTM_ERR_INVALID; }
    for (int k = 0; k < d->n_kf; ++k)
        if (!same_geometry(d->kf[k])) { set_err(ctx, "track: keyframe %d is NULL, foreign or of another geometry", k); return DSDTM_ERR_INVALID; }
    if (int rc = validate_params(ctx, &d->align, pl.levels)) return rc;
    const int M = d->n_points;
    const int nnz = M > 0 ? d->obs_offset[M] : 0;
    out->nnz = nnz; out->max_search_level = max_search_level;
    out->frames_seq = d->ref->seq;
    for (int k = 0; k < d->n_kf; ++k) if (d->kf[k]->seq > out->frames_seq) out->frames_seq = d->kf[k]->seq;
    if (M > 0) {
        if (d->obs_offset[0] != 0 || nnz < 0 || (nnz > 0 && (!d->obs_kf || !d->obs_px || !d->obs_level || !d->obs_bearing))) {
            set_err(ctx, "track: bad observation arrays"); return DSDTM_ERR_INVALID;
        }
        for (int i = 0; i < M; ++i)
            if (d->obs_offset[i + 1] < d->obs_offset[i]) { set_err(ctx, "track: obs_offset is not monotone at point %d", i); return DSDTM_ERR_INVALID; }
        for (int j = 0; j < nnz; ++j)
            if (d->obs_kf[j] < 0 || d->obs_kf[j] >= d->n_kf || d->obs_level[j] < 0 || d->obs_level[j] >= pl.levels) {
                set_err(ctx, "track: observation %d names keyframe %d / level %d out of range", j, d->obs_kf[j], d->obs_level[j]);
                return DSDTM_ERR_INVALID;
            }
    }
    const int grid_rows = (d->height + d->cell_size - 1) / d->cell_size, grid_cols = (d->width + d->cell_size - 1) / d->cell_size;   // :29-30
    if ((long long)grid_rows * grid_cols > 4096) { set_err(ctx, "track: more than 4096 grid cells"); return DSDTM_ERR_INVALID; }
    const size_t lds = track_replay_lds_bytes(M, grid_rows * grid_cols, d->cell_size);
    if (lds > 160 * 1024 - 256) { set_err(ctx, "track: %d map points over %d cells do not fit one workgroup's LDS", M, grid_rows * grid_cols); return DSDTM_ERR_INVALID; }
    out->grid_rows = grid_rows; out->grid_cols = grid_cols;
    return DSDTM_OK;
}

// ---- the staging of a tracked call, and what both entries do with it ---------------------------------------------
// Offsets into the pinned block (h_*: host-mapped) and into the device scratch (g_*). Each entry fills it in its own order and they
// share the names: the single call's layout is the batch's with one frame and as many columns as map points; unused members stay 0.
struct TrackLayout {
    size_t h_img;                                                    // staged images
    // Run's range (what it reads, then its in/out pose, count and statistics): moved to the device in one piece
    size_t h_run, h_px, h_bear, h_pw, h_ini, h_nf, h_tr, h_rp, h_cp, h_T, h_nt, h_st, run_bytes, run_out_bytes;
    // the local map(s) and mask(s): one contiguous range, copied to the device in one piece
    size_t h_map, h_mask, h_fmask, h_bf, h_c0, h_np, h_mpw, h_found, h_bad, h_off, h_okf, h_opx, h_olv, h_ob, h_Tkf, h_kfp, map_bytes;
    size_t h_cnt, h_match, h_Topt, h_sm, h_rn, h_grid, h_total;      // results the kernels post straight into the pinned block
    size_t g_run, g_map, g_pw, g_cell, g_px0, g_px, g_ck, g_cf, g_rpx, g_rl, g_rb, g_ib, g_sl, g_cv, g_grid, g_pob, g_pow, g_pol, g_pou,
           g_pon, g_Topt, g_total;
};

// The arguments of the kernels behind Run — reprojection + FindMatchDirect, the replay, the pose refinement — from the layout.
// g / hd: the device scratch and the pinned block as the device sees it; d: search parameters of every frame; columns / n_kf: over
// all frames. The caller then sets what is its own: dsdtm_track_frame the mask and run_out_n16, dsdtm_track_frames the per-frame tables.
static void bind_track_kernels(const TrackLayout& L, uint8_t* g, uint8_t* hd, const dsdtm_camera* cam, const dsdtm_track_desc* d,
                               const TrackPlan& plan, int n_frames, int columns, int n_kf, const uint8_t* cur_pyr, size_t pitch,
                               TrackArgs& t, WarpKernelArgs& wa, A2DKernelArgs& aa, PoseOptArgs& pa) {
    const PackedPyr& pl = plan.pl;
    uint8_t* const gr = g + L.g_run - L.h_run;          // device address of the pinned block's offset X inside Run's range: gr + X
    const uint8_t* gm = g + L.g_map - L.h_map;          // ... inside the map range: gm + X
    memset(&t, 0, sizeof t);
    t.T_run = (const double*)(gr + L.h_T); t.n_tracked = (const int32_t*)(gr + L.h_nt); t.min_tracked = d->min_tracked;
    t.run_out_dev = gr + L.h_T; t.run_out_host = hd + L.h_T;
    t.T_kf_w = (const double*)(gm + L.h_Tkf); t.kf_ptrs = (const uint8_t* const*)(gm + L.h_kfp); t.n_kf = n_kf;
    t.mp_world = (const double*)(gm + L.h_mpw); t.mp_found = (const int32_t*)(gm + L.h_found); t.mp_bad = gm + L.h_bad; t.n_points = columns;
    t.obs_offset = (const int32_t*)(gm + L.h_off); t.obs_kf = (const int32_t*)(gm + L.h_okf); t.obs_px = (const float*)(gm + L.h_opx);
    t.obs_level = (const int32_t*)(gm + L.h_olv); t.obs_bearing = (const double*)(gm + L.h_ob);
    t.mask = nullptr; t.mask_stride = d->width;
    t.fx = cam->fx; t.fy = cam->fy; t.cx = cam->cx; t.cy = cam->cy; t.width = cam->width; t.height = cam->height; t.levels = pl.levels;
    t.cell_size = d->cell_size; t.grid_cols = plan.grid_cols; t.grid_rows = plan.grid_rows; t.max_matches = d->max_matches;
    track_disc_half_widths(d->cell_size, t.disc_hw);
    t.pw = (double*)(g + L.g_pw); t.cell = (int32_t*)(g + L.g_cell); t.px0 = (double*)(g + L.g_px0); t.px = (double*)(g + L.g_px);
    t.cand_kf = (int32_t*)(g + L.g_ck); t.cand_frame = (int32_t*)(g + L.g_cf); t.ref_px = (float*)(g + L.g_rpx); t.ref_level = (int32_t*)(g + L.g_rl);
    t.ref_bearing = (double*)(g + L.g_rb); t.init_blocked = g + L.g_ib; t.search_level = (int32_t*)(g + L.g_sl); t.converged = g + L.g_cv;
    t.matches = (dsdtm_track_match*)(hd + L.h_match); t.counts = (int32_t*)(hd + L.h_cnt); t.T_opt = (double*)(g + L.g_Topt);
    t.po_bearing = (double*)(g + L.g_pob); t.po_world = (double*)(g + L.g_pow); t.po_level = (int32_t*)(g + L.g_pol); t.po_use = g + L.g_pou;
    t.po_n = (int32_t*)(g + L.g_pon);
    memset(&wa, 0, sizeof wa);
    fill_levels(wa.lv, pl, pl.levels);
    wa.kf_ptrs = t.kf_ptrs; wa.T_kf_w = t.T_kf_w; wa.T_cur_w_arr = t.T_run; wa.cand_frame = t.cand_frame;
    wa.cand_kf = t.cand_kf; wa.ref_px = t.ref_px; wa.ref_level = t.ref_level; wa.ref_bearing = t.ref_bearing; wa.p_world = t.pw;
    wa.search_level = t.search_level; wa.m = columns; wa.n_kf = n_kf; wa.max_search_level = plan.max_search_level; wa.levels = pl.levels;
    wa.n_frames = n_frames; wa.fx = cam->fx; wa.fy = cam->fy; wa.cx = cam->cx; wa.cy = cam->cy; wa.no_xcd = options().fmd_no_xcd;
    memset(&aa, 0, sizeof aa);
    aa.cur_pyr = cur_pyr; aa.level = t.search_level; aa.px_xy = t.px; aa.converged = t.converged; aa.m = columns; aa.max_iters = d->align2d_iters;
    aa.levels = pl.levels; aa.px_level0 = 1; aa.frame = t.cand_frame; aa.n_frames = n_frames; aa.pyr_pitch = pitch;
    for (int l = 0; l < pl.levels; ++l) aa.lv[l] = wa.lv[l];
    pa.n_frames = n_frames; pa.max_features = d->max_matches; pa.max_iterations = d->pose_opt.max_iterations;
    pa.n_features = t.po_n; pa.bearing = t.po_bearing; pa.p_world = t.po_world; pa.level = t.po_level; pa.use = t.po_use;
    pa.T_cur_w = t.T_opt; pa.T_mirror = (double*)(hd + L.h_Topt); pa.residual_norm = (double*)(hd + L.h_rn); pa.summary = (dsdtm_pose_opt_summary*)(hd + L.h_sm);
    pa.force_variant = 3;                              // one wave / four waves per frame by its match count, chosen by the kernel
}

// The results of the frame in slot `slot` out of the pinned block h, behind the wait. stride: matches per frame in the block.
// false: the replay of the frame's cell walk did not settle — nothing behind replay_full_scan is read (the caller reports it).
static bool read_track_result(const uint8_t* h, const TrackLayout& L, size_t slot, size_t stride, int min_tracked, dsdtm_track_result* res,
                              dsdtm_track_match* matches, double* residual_norm) {
    memcpy(res->T_run, h + L.h_T + slot * 96, 96);
    res->n_tracked = ((const int32_t*)(h + L.h_nt))[slot];
    memcpy(&res->stats, h + L.h_st + slot * sizeof(dsdtm_align_stats), sizeof res->stats);
    res->lost = res->n_tracked < min_tracked ? 1 : 0;
    const int32_t* cnt = (const int32_t*)(h + L.h_cnt) + 4 * slot;
    res->n_in_grid = cnt[0];
    res->n_matches = res->lost ? 0 : cnt[1];
    res->replay_full_scan = cnt[2] == 1 ? 1 : 0;
    if (cnt[2] == 2 && !res->lost) return false;
    if (res->lost) memcpy(res->T_opt, res->T_run, 96);
    else {
        memcpy(res->T_opt, h + L.h_Topt + slot * 96, 96);
        memcpy(&res->summary, h + L.h_sm + slot * sizeof(dsdtm_pose_opt_summary), sizeof res->summary);
        if (res->n_matches > 0) memcpy(matches, h + L.h_match + slot * stride * sizeof(dsdtm_track_match), (size_t)res->n_matches * sizeof(dsdtm_track_match));
        if (res->summary.n_residual_blocks > 0) memcpy(residual_norm, h + L.h_rn + slot * stride * 8, (size_t)res->summary.n_residual_blocks * 8);
    }
    return true;
}

// ---- one tracked frame in ONE submission (src/Tracking.cpp:199-256) ------------------------------
// new frame -> Run -> ReprojectPoint + Get_ClosetObs for every local map point -> FindMatchDirect for all of them -> the cell
// walk of SearchLocalPoints replayed on the device -> PoseOptimization, enqueued back to back on the context's stream; the host
// waits once. What crosses the link crosses it once and off the kernels' critical paths: level 0 and Run's inputs are read from
// host-mapped pinned memory by ONE kernel into HBM, the local map goes up on a second stream while Run runs, every later kernel
// works on device memory and the few results are written (posted) to the pinned block by whichever kernel has them first.
// cur == NULL: dsdtm_track_frame — the new frame is made here from d->image. cur != NULL: dsdtm_track_frame_on — the frame is
// already on the device (or on its way there: the stream waits for its event); the chain starts at Run.
// (No heap allocation on this path: its state is on the stack.)
static int track_frame_impl(dsdtm_ctx* ctx, const dsdtm_camera* cam, const dsdtm_track_desc* d, dsdtm_frame* cur, dsdtm_track_result* res,
                            dsdtm_track_match* matches, double* residual_norm) {
    memset(res, 0, sizeof *res);
    TrackPlan plan;
    if (cur) {
        if (cur->owner != ctx) { set_err(ctx, "track_frame_on: cur belongs to another context"); return DSDTM_ERR_INVALID; }
        if (d->image) { set_err(ctx, "track_frame_on: desc->image must be NULL (the frame is already on the device)"); return DSDTM_ERR_INVALID; }
        if (cur->pl.levels != d->levels || cur->pl.w[0] != d->width || cur->pl.h[0] != d->height) {
            set_err(ctx, "track_frame_on: desc->width / height / levels (%dx%d, %d) are not the frame's (%dx%d, %d)", d->width, d->height,
                    d->levels, cur->pl.w[0], cur->pl.h[0], cur->pl.levels);
            return DSDTM_ERR_INVALID;
        }
    }
    if (int rc = track_check_desc(ctx, cam, d, &plan, cur != nullptr)) return rc;
    if (cur) {
        const PackedPyr& q = cur->pl;
        if (memcmp(q.w, plan.pl.w, sizeof(int) * q.levels) || memcmp(q.h, plan.pl.h, sizeof(int) * q.levels)) {   // (a frame from dsdtm_frame_create with levels of its own)
            set_err(ctx, "track_frame_on: desc->width / height / levels (%dx%d, %d) are not the frame's (%dx%d, %d)", d->width, d->height,
                    d->levels, q.w[0], q.h[0], q.levels);
            return DSDTM_ERR_INVALID;
        }
        if (cur->seq > plan.frames_seq) plan.frames_seq = cur->seq;
    }
    const PackedPyr& pl = plan.pl;
    const int M = d->n_points, nnz = plan.nnz;
    const size_t img = (size_t)d->width * d->height, nf = (size_t)d->n_ref_features, Mz = (size_t)M, NZ = (size_t)nnz,
                 MM = (size_t)d->max_matches, NK = (size_t)d->n_kf;
    TrackLayout L = {};
    {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
        L.h_img = take(img);
        L.h_run = o;
        L.h_bear = take(nf * 24); L.h_pw = take(nf * 24); L.h_tr = take(96); L.h_px = take(nf * 8); L.h_ini = take(nf);
        L.h_T = take(96); L.h_nt = take(4); L.h_st = take(sizeof(dsdtm_align_stats));
        L.run_bytes = o - L.h_run; L.run_out_bytes = o - L.h_T;
        L.h_map = o;
        L.h_mask = take(d->mask ? img : 0);
        L.h_mpw = take(Mz * 24); L.h_found = take(Mz * 4); L.h_bad = take(Mz); L.h_off = take((Mz + 1) * 4); L.h_okf = take(NZ * 4);
        L.h_opx = take(NZ * 8); L.h_olv = take(NZ * 4); L.h_ob = take(NZ * 24); L.h_Tkf = take(NK * 96); L.h_kfp = take(NK * sizeof(void*));
        L.map_bytes = o - L.h_map;
        L.h_cnt = take(64); L.h_match = take(MM * sizeof(dsdtm_track_match)); L.h_Topt = take(96); L.h_sm = take(sizeof(dsdtm_pose_opt_summary));
        L.h_rn = take(MM * 8); L.h_total = o;
        o = 0;
        L.g_run = take(L.run_bytes); L.g_map = take(L.map_bytes); L.g_pw = take(Mz * 24); L.g_cell = take(Mz * 4);
        L.g_px0 = take(Mz * 16); L.g_px = take(Mz * 16); L.g_ck = take(Mz * 4); L.g_cf = take(Mz * 4); L.g_rpx = take(Mz * 8);
        L.g_rl = take(Mz * 4); L.g_rb = take(Mz * 24); L.g_ib = take(Mz); L.g_sl = take(Mz * 4); L.g_cv = take(Mz);
        L.g_pob = take(MM * 24); L.g_pow = take(MM * 24); L.g_pol = take(MM * 4); L.g_pou = take(MM); L.g_pon = take(4); L.g_Topt = take(96);
        L.g_total = o;
    }
    if (int rc = ensure_stage(ctx, L.h_total > L.g_total ? L.h_total : L.g_total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    uint8_t* hd = nullptr;                             // the pinned block as the device sees it
    if (int rc = pinned_device_ptr(ctx, &hd)) return rc;
    hipStream_t stream = ctx->stream;
    dsdtm_frame* f = cur;
    if (!cur) { if (int rc = frame_alloc(ctx, pl, stream, &f)) return rc; }
    auto fail = [&](int rc) {
        if (ctx->copy_stream[0]) (void)hipStreamSynchronize(ctx->copy_stream[0]);
        (void)hipStreamSynchronize(stream);
        if (!cur) dsdtm_frame_destroy(ctx, f);          // (a frame the caller handed in stays the caller's)
        return rc;
    };
    // 1. the new frame: level 0 crosses the link, the pyramid is built on the device (src/Frame.cpp:35-41, :74-81); with it
    //    what Run(cur, ref) reads and its in/out pose: ONE kernel (ingest_kernel, pyrdown.hip) on the compute stream reads both
    //    from host-mapped pinned memory — no copy operation in front of the first kernel (the hand-over from the copy engine
    //    costs 7-8 us), and Run reads its 57 bytes per feature from HBM instead of over the link.
    // (an image in pinned memory — e.g. the capture buffer — or in this device's memory is read from there; anything else is
    // staged through the context's pinned block first: 5-15 us of host memcpy for 640x480. The routes: ImageRoute)
    ImageRoute route = {IN_PLACE, nullptr, 0};
    if (!cur) {
        route = route_image(ctx, d->image, d->width, d->stride, false);
        if (route.route == OTHER_DEVICE) { set_err(ctx, "track: the image lives on device %d, the context on %d", route.device, ctx->device); return fail(DSDTM_ERR_INVALID); }
        if (route.route == STAGED) {
            copy_rows(h + L.h_img, (size_t)d->width, d->image, (size_t)d->stride, (size_t)d->width, (size_t)d->height);
            route.dev = hd + L.h_img;
        }
    }
    if (nf) {
        memcpy(h + L.h_bear, d->ref_bearing, nf * 24); memcpy(h + L.h_pw, d->ref_p_world, nf * 24);
        memcpy(h + L.h_px, d->ref_px_xy, nf * 8); memcpy(h + L.h_ini, d->ref_initial, nf);
    }
    memcpy(h + L.h_tr, d->T_ref_w, 96);
    auto seed_run = [&]() {
        memcpy(h + L.h_T, d->T_seed, 96);                            // cur->Set_Pose(last->Get_Pose()) (src/Tracking.cpp:201)
        memset(h + L.h_nt, 0, 4); memset(h + L.h_st, 0, sizeof(dsdtm_align_stats));
    };
    seed_run();
    if (int rc = frames_consume(ctx, plan.frames_seq, stream)) return fail(rc);      // pending frames among ref / kf / cur
    const RunRange run_range = {hd + L.h_run, g + L.g_run, L.run_bytes};
    if (cur) API_TRY(ingest_launch(nullptr, nullptr, 0, run_range.src, run_range.dst, run_range.bytes, stream));   // Run's range only
    else {
        if (int rc = enqueue_level0(ctx, route, d->image, d->width, d->height, d->stride, f->d, &run_range, stream)) return fail(rc);
        if (int rc = dsdtm_pyrdown_batch_device(ctx, f->d, f->pitch, 1, pl.levels, pl.w, pl.h, plan.st, pl.off, stream)) return fail(rc);
    }

    // 2. Run(cur, ref) on the device copy of its range
    // Run() (:34-38): too few features -> 0, the pose untouched. Decided on the host: no launch.
    const bool run = d->n_ref_features >= d->align.min_fts && d->align.max_level - 1 >= d->align.min_level && d->n_ref_features > 0;
    uint8_t* const gr = g + L.g_run - L.h_run;          // device address of the pinned block's offset X inside Run's range: gr + X
    dsdtm_batch_desc b;
    memset(&b, 0, sizeof b);
    b.n_pairs = 1; b.max_features = d->n_ref_features;
    fill_levels(b, pl);
    b.pyr_pitch = d->ref->pitch;
    b.ref_pyr = d->ref->d; b.cur_pyr = f->d;
    b.px_xy = (const float*)(gr + L.h_px); b.bearing = (const double*)(gr + L.h_bear); b.p_world = (const double*)(gr + L.h_pw);
    b.initial = gr + L.h_ini; b.T_ref_w = (const double*)(gr + L.h_tr); b.T_cur_w = (double*)(gr + L.h_T);
    b.n_tracked = (int32_t*)(gr + L.h_nt); b.stats = (dsdtm_align_stats*)(gr + L.h_st);
    if (d->ref->pitch != f->pitch) { set_err(ctx, "track: pyramid pitches differ"); return fail(DSDTM_ERR_INVALID); }

    // 3. the local map, packed once (the retry below re-uses it)
    bool packed_map = false;
    auto pack_map = [&]() {
        if (packed_map) return;
        packed_map = true;
        if (d->mask) copy_rows(h + L.h_mask, (size_t)d->width, d->mask, (size_t)d->mask_stride, (size_t)d->width, (size_t)d->height);
        if (M > 0) {
            memcpy(h + L.h_mpw, d->mp_world, Mz * 24); memcpy(h + L.h_found, d->mp_found, Mz * 4); memcpy(h + L.h_bad, d->mp_bad, Mz);
            memcpy(h + L.h_off, d->obs_offset, (Mz + 1) * 4);
        } else memset(h + L.h_off, 0, 4);
        if (nnz > 0) {
            memcpy(h + L.h_okf, d->obs_kf, NZ * 4); memcpy(h + L.h_opx, d->obs_px, NZ * 8); memcpy(h + L.h_olv, d->obs_level, NZ * 4);
            memcpy(h + L.h_ob, d->obs_bearing, NZ * 24);
        }
        if (d->n_kf > 0) memcpy(h + L.h_Tkf, d->T_kf_w, NK * 96);
        for (int k = 0; k < d->n_kf; ++k) ((const uint8_t**)(h + L.h_kfp))[k] = d->kf[k]->d;
    };

    TrackArgs t; WarpKernelArgs wa; A2DKernelArgs aa; PoseOptArgs pa;
    bind_track_kernels(L, g, hd, cam, d, plan, 1, M, d->n_kf, f->d, f->pitch, t, wa, aa, pa);
    t.mask = d->mask ? g + L.g_map - L.h_map + L.h_mask : nullptr;
    // (Run's pose, count and statistics reach the pinned block by the match kernel's posted writes: no copy operation on the chain)
    t.run_out_n16 = (int)(L.run_out_bytes / 16);
    volatile unsigned* h_flag = ctx->h_flags + dsdtm_ctx::FLAG_SINGLE;
    *h_flag = 0;
    LaunchMode mode;
    mode.single = true;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool multi_cu = false;
        if (attempt) {                                               // once more: Run's range again, from the seed
            seed_run();
            API_TRY(ingest_launch(nullptr, nullptr, 0, run_range.src, run_range.dst, run_range.bytes, stream));
        }
        memset(h + L.h_cnt, 0, 64); memset(h + L.h_sm, 0, sizeof(dsdtm_pose_opt_summary));
        if (run) { if (int rc = launch_batch(ctx, &b, cam, &d->align, stream, mode, &multi_cu)) return fail(rc); }
        if (!packed_map) {
            // the local map does not depend on Run: it is packed and copied up on a second stream WHILE Run runs (its reads —
            // observation -> keyframe pose -> reference feature — are dependent chains: from host-mapped memory they cost the
            // reprojection 16 us, from HBM 4)
            pack_map();
            if (!ctx->copy_stream[0]) API_TRY(hipStreamCreateWithFlags(&ctx->copy_stream[0], hipStreamNonBlocking));
            API_TRY(hipMemcpyAsync(g + L.g_map, h + L.h_map, L.map_bytes, hipMemcpyHostToDevice, ctx->copy_stream[0]));
            // (waited for by the HOST, while Run runs: a device-side event wait costs the stream a 6-us bubble in front of the
            // next kernel; the kernels behind Run are still enqueued long before Run ends)
            API_TRY(hipStreamSynchronize(ctx->copy_stream[0]));
        }
        // 4. ReprojectPoint + Get_ClosetObs for every point; FindMatchDirect for every point that passed; the cell walk; the
        //    features of the matches; PoseOptimization on them — the instantiation picked on the device by the match count,
        //    as dsdtm_pose_optimization picks it on the host (same arithmetic, same bits as the four-call chain)
        API_TRY(track_match_launch(t, wa, aa, stream));
        API_TRY(track_replay_launch(t, stream));
        API_TRY(pose_opt_launch(pa, stream));
        API_TRY(hipStreamSynchronize(stream));
        frames_settle(ctx);
        if (!*h_flag) break;
        *h_flag = 0;
        if (!multi_cu || attempt == 1 || options().no_recover) {
            clear_stream_counters(ctx, ctx->stream);
            set_err(ctx, multi_cu ? "sparse-align kernel: a wait for a partner workgroup timed out (re-run disabled: no_recover)"
                                  : "sparse-align kernel: intra-workgroup hand-over timed out");
            return fail(DSDTM_ERR_HIP);
        }
        mode.one_cu = true;                                          // Run cannot fail for scheduling reasons: once more, on one compute unit
        ctx->recovered += 1;
    }
    res->frame = f;
    if (!read_track_result(h, L, 0, MM, d->min_tracked, res, matches, residual_norm)) {
        set_err(ctx, "track: the replay of the cell walk did not settle"); if (!cur) dsdtm_frame_destroy(ctx, f); res->frame = nullptr; return DSDTM_ERR_HIP;
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_track_frame(dsdtm_ctx* ctx, const dsdtm_camera* cam, const dsdtm_track_desc* d, dsdtm_track_result* res,
                                 dsdtm_track_match* matches, double* residual_norm) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam || !d || !res || !matches || !residual_norm) { set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID; }
    return track_frame_impl(ctx, cam, d, nullptr, res, matches, residual_norm);
}

extern "C" int dsdtm_track_frame_on(dsdtm_ctx* ctx, const dsdtm_camera* cam, const dsdtm_track_desc* d, dsdtm_frame* cur,
                                    dsdtm_track_result* res, dsdtm_track_match* matches, double* residual_norm) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam || !d || !cur || !res || !matches || !residual_norm) {
        set_err(ctx, "track_frame_on: NULL argument (%s)", !cam ? "cam" : !d ? "desc" : !cur ? "cur" : !res ? "result" : !matches ? "matches" : "residual_norm");
        return DSDTM_ERR_INVALID;
    }
    return track_frame_impl(ctx, cam, d, cur, res, matches, residual_norm);
}

// ---- n independent tracked frames in ONE submission ------------------------------------------------
// dsdtm_track_frame for n frames of n independent trackers: every stage runs once for the whole batch — ingest of the n images
// into ONE slab of packed pyramids (frame slot s at s * pitch) and the pyramid kernel over all of them; Run once per register
// band present (the instantiation each frame's single call would run, its reference pyramid through a pointer table); the
// reprojection + FindMatchDirect kernel over the columns of all frames (one frame per workgroup); the replay of the cell walk,
// one workgroup per frame; the pose refinement, one instantiation per frame by its match count. The host waits once.
// Inside the call frames sit in SLOT order — sorted by register band, so that each band's pairs are contiguous in the Run
// arrays and in the slab — and are handed back in the caller's order.
// RESIDENT MODE (descs[f].image == NULL for every f): the new frames are already on the device, or on their way there —
// results[f].frame names frame f on entry (dsdtm_frame_prefetch, pending or not; dsdtm_frame_create_from_image; a member of an
// earlier call's slab). No slab, no ingest of images, no pyramid kernel: the chain starts at Run, behind a device-side wait for
// the latest prefetch among all frames named. The frames are separate allocations in the caller's order, so Run and the
// FindMatchDirect kernel find slot s's current pyramid through a table (cur_ptrs, in Run's range beside ref_ptrs). The frames
// stay the caller's: results[f].frame is the same pointer on return, on success and on every failure.
// The entry is a sequence of phases (tracks_*), each with one job; TrackBatch is what they hand on.
static int track_band(const dsdtm_track_desc* d) {
    const bool run = d->n_ref_features >= d->align.min_fts && d->align.max_level - 1 >= d->align.min_level && d->n_ref_features > 0;
    if (!run) return 7;                                            // no Run launch (the Min_fts rule, as the single call)
    switch (sparse_align_pick_variant(d->n_ref_features)) {
        case SA_REG128: return 0;
        case SA_REG192: return 1;
        case SA_REG256: return 2;
        case SA_REG320: return 3;
        case SA_REG448: return 4;
        default: return 5;                                         // SA_REG704 (n_ref_features <= 704 is checked)
    }
}
static const SAVariant kBandVariant[6] = {SA_REG128, SA_REG192, SA_REG256, SA_REG320, SA_REG448, SA_REG704};

struct TrackBatch {
    int n; bool resident; const dsdtm_camera* cam; const dsdtm_track_desc* descs;
    std::vector<dsdtm_frame*> cur;           // resident mode: the frames, in the caller's order
    std::vector<TrackPlan> plans;            // per frame
    std::vector<ImageRoute> route;           // per frame (image mode)
    std::vector<int> order;                  // slot -> frame
    std::vector<int32_t> col0, blk_frame;    // per slot: its first column; per match workgroup: its slot
    int band_lo[9];                          // slots of band b: [band_lo[b], band_lo[b + 1])
    size_t MF, C, NZ, NK, NMASK, NB, n_staged, pitch, img, img_pitch, MM;   // MF: feature stride; columns, observations, keyframes, masks, match workgroups, staged images over all frames
    int max_points;
    TrackLayout L;
    uint8_t *h, *g, *hd, *slab;              // the pinned block, the device scratch, the block as the device sees it; image mode: the new frames
};

// every frame is checked before anything is allocated or enqueued
static int tracks_check(dsdtm_ctx* ctx, TrackBatch& B) {
    const int n = B.n;
    const bool resident = B.resident; const std::vector<dsdtm_frame*>& cur = B.cur;
    try { B.plans.resize((size_t)n); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
    const dsdtm_track_desc& d0 = B.descs[0];
    for (int f = 0; f < n; ++f) {
        const dsdtm_track_desc* d = &B.descs[f];
        const char* field = nullptr;
        if (d->width != d0.width) field = "width";
        else if (d->height != d0.height) field = "height";
        else if (d->levels != d0.levels) field = "levels";
        else if (d->align.max_level != d0.align.max_level || d->align.min_level != d0.align.min_level ||
                 d->align.max_iters != d0.align.max_iters || d->align.min_fts != d0.align.min_fts) field = "align";
        else if (d->min_tracked != d0.min_tracked) field = "min_tracked";
        else if (d->cell_size != d0.cell_size) field = "cell_size";
        else if (d->max_pyr_levels != d0.max_pyr_levels) field = "max_pyr_levels";
        else if (d->max_matches != d0.max_matches) field = "max_matches";
        else if (d->align2d_iters != d0.align2d_iters) field = "align2d_iters";
        else if (d->pose_opt.max_iterations != d0.pose_opt.max_iterations) field = "pose_opt";
        if (field) { set_err(ctx, "track_frames: frame %d: %s differs from frame 0 (shared across the batch)", f, field); return DSDTM_ERR_INVALID; }
        if (resident) {
            const dsdtm_frame* c = cur[(size_t)f];
            if (!c) { set_err(ctx, "track_frames: frame %d: results[%d].frame is NULL (image is NULL: the frame must already be on the device)", f, f); return DSDTM_ERR_INVALID; }
            if (c->owner != ctx || c->device != ctx->device) { set_err(ctx, "track_frames: frame %d: results[%d].frame belongs to another context", f, f); return DSDTM_ERR_INVALID; }
            const char* geom = c->pl.w[0] != d->width ? "width" : c->pl.h[0] != d->height ? "height" : c->pl.levels != d->levels ? "levels" : nullptr;
            if (geom) {
                set_err(ctx, "track_frames: frame %d: desc %s (%dx%d, %d levels) is not results[%d].frame's (%dx%d, %d levels)", f, geom, d->width,
                        d->height, d->levels, f, c->pl.w[0], c->pl.h[0], c->pl.levels);
                return DSDTM_ERR_INVALID;
            }
            if (c == d->ref) { set_err(ctx, "track_frames: frame %d: ref is results[%d].frame itself", f, f); return DSDTM_ERR_INVALID; }
        }
        if (int rc = track_check_desc(ctx, B.cam, d, &B.plans[(size_t)f], resident)) {
            char msg[sizeof ctx->err];
            snprintf(msg, sizeof msg, "%s", ctx->err);
            set_err(ctx, "track_frames: frame %d: %s", f, msg);
            return rc;
        }
        if (d->n_ref_features > 704) { set_err(ctx, "track_frames: frame %d: %d reference features (at most 704)", f, d->n_ref_features); return DSDTM_ERR_INVALID; }
        if (d->ref->pitch != align_up(B.plans[(size_t)f].pl.bytes, 256)) { set_err(ctx, "track_frames: frame %d: pyramid pitches differ", f); return DSDTM_ERR_INVALID; }
        if (resident) {
            const dsdtm_frame* c = cur[(size_t)f];
            const PackedPyr& q = B.plans[(size_t)f].pl;
            // (a frame from dsdtm_frame_create with levels or a pitch of its own)
            if (memcmp(c->pl.w, q.w, sizeof(int) * q.levels) || memcmp(c->pl.h, q.h, sizeof(int) * q.levels) || memcmp(c->pl.off, q.off, sizeof(q.off[0]) * q.levels) ||
                c->pitch != d->ref->pitch) {
                set_err(ctx, "track_frames: frame %d: levels of results[%d].frame are not those of a %dx%d image with %d levels", f, f, d->width, d->height, d->levels);
                return DSDTM_ERR_INVALID;
            }
            if (c->seq > B.plans[(size_t)f].frames_seq) B.plans[(size_t)f].frames_seq = c->seq;
        }
    }
    if (resident) {                                                // the same frame twice: named by its later place in the call
        std::vector<std::pair<const dsdtm_frame*, int>> by_ptr;
        try { for (int f = 0; f < n; ++f) by_ptr.emplace_back(cur[(size_t)f], f); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
        std::sort(by_ptr.begin(), by_ptr.end());
        int dup = -1, first = -1;
        for (size_t i = 1; i < by_ptr.size(); ++i)
            if (by_ptr[i].first == by_ptr[i - 1].first && (dup < 0 || by_ptr[i].second < dup)) { dup = by_ptr[i].second; first = by_ptr[i - 1].second; }
        if (dup >= 0) { set_err(ctx, "track_frames: frame %d: results[%d].frame is also frame %d's (a frame at most once per call)", dup, dup, first); return DSDTM_ERR_INVALID; }
    }
    return DSDTM_OK;
}

// slot order: by register band (stable); sizes: columns (each frame padded to whole match workgroups, at least one),
// observations, keyframes, masks
static int tracks_order_and_sizes(dsdtm_ctx* ctx, TrackBatch& B) {
    const int n = B.n;
    const dsdtm_track_desc& d0 = B.descs[0];
    B.pitch = align_up(B.plans[0].pl.bytes, 256); B.img = (size_t)d0.width * d0.height; B.MM = (size_t)d0.max_matches;
    std::vector<int> band;
    try { B.order.resize((size_t)n); band.resize((size_t)n); B.col0.resize((size_t)n); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
    int* band_lo = B.band_lo;
    memset(band_lo, 0, sizeof B.band_lo);
    for (int f = 0; f < n; ++f) { band[(size_t)f] = track_band(&B.descs[f]); band_lo[band[(size_t)f] + 1]++; }
    for (int b = 0; b < 8; ++b) band_lo[b + 1] += band_lo[b];
    {
        int next[8];
        for (int b = 0; b < 8; ++b) next[b] = band_lo[b];
        for (int f = 0; f < n; ++f) B.order[(size_t)next[band[(size_t)f]]++] = f;
    }
    B.MF = 1; B.C = B.NZ = B.NK = B.NMASK = 0; B.max_points = 0;
    for (int s = 0; s < n; ++s) {
        const dsdtm_track_desc* d = &B.descs[B.order[(size_t)s]];
        if ((size_t)d->n_ref_features > B.MF) B.MF = (size_t)d->n_ref_features;
        B.col0[(size_t)s] = (int32_t)B.C;
        const size_t groups = d->n_points > 0 ? ((size_t)d->n_points + TRACK_COL_GROUP - 1) / TRACK_COL_GROUP : 1;
        try { for (size_t g = 0; g < groups; ++g) B.blk_frame.push_back(s); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
        B.C += groups * TRACK_COL_GROUP;
        B.NZ += (size_t)B.plans[(size_t)B.order[(size_t)s]].nnz;
        B.NK += (size_t)d->n_kf;
        if (d->mask) B.NMASK++;
        if (d->n_points > B.max_points) B.max_points = d->n_points;
    }
    B.NB = B.blk_frame.size();
    return DSDTM_OK;
}

// the pinned block and the device scratch; how every image travels (which sizes the staging of pageable images); the staging itself
static int tracks_layout(dsdtm_ctx* ctx, TrackBatch& B) {
    const size_t NF = (size_t)B.n, MF = B.MF, C = B.C, NZ = B.NZ, NK = B.NK, MM = B.MM;
    TrackLayout& L = B.L;
    memset(&L, 0, sizeof L);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
    // Run's range (slot order, features at stride MF): inputs, then the poses / counts / statistics Run writes
    L.h_run = o;
    L.h_px = take(NF * MF * 8); L.h_bear = take(NF * MF * 24); L.h_pw = take(NF * MF * 24); L.h_ini = take(NF * MF);
    L.h_nf = take(NF * 4); L.h_tr = take(NF * 96); L.h_rp = take(NF * sizeof(void*)); L.h_cp = take(B.resident ? NF * sizeof(void*) : 0);
    L.h_T = take(NF * 96); L.h_nt = take(NF * 4); L.h_st = take(NF * sizeof(dsdtm_align_stats));
    L.run_bytes = o - L.h_run; L.run_out_bytes = o - L.h_T;
    // the local maps and masks (slot order, columns padded): one range, copied up in one piece
    L.h_map = o;
    L.h_mask = take(B.NMASK * B.img); L.h_fmask = take(NF * sizeof(void*)); L.h_bf = take(B.NB * 4); L.h_c0 = take(NF * 4);
    L.h_np = take(NF * 4); L.h_mpw = take(C * 24); L.h_found = take(C * 4); L.h_bad = take(C); L.h_off = take((C + 1) * 4);
    L.h_okf = take(NZ * 4); L.h_opx = take(NZ * 8); L.h_olv = take(NZ * 4); L.h_ob = take(NZ * 24); L.h_Tkf = take(NK * 96);
    L.h_kfp = take(NK * sizeof(void*));
    L.map_bytes = o - L.h_map;
    // results the kernels post straight into the pinned block
    L.h_cnt = take(NF * 16); L.h_match = take(NF * MM * sizeof(dsdtm_track_match)); L.h_Topt = take(NF * 96);
    L.h_sm = take(NF * sizeof(dsdtm_pose_opt_summary)); L.h_rn = take(NF * MM * 8); L.h_grid = take(C);
    // pageable host images are staged here
    B.n_staged = 0;
    try { B.route.resize(NF); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
    for (int f = 0; f < B.n && !B.resident; ++f) {
        const dsdtm_track_desc* d = &B.descs[f];
        B.route[(size_t)f] = route_image(ctx, d->image, d->width, d->stride, true);
        if (B.route[(size_t)f].route == OTHER_DEVICE) { set_err(ctx, "track_frames: frame %d: the image lives on device %d, the context on %d", f, B.route[(size_t)f].device, ctx->device); return DSDTM_ERR_INVALID; }
        if (B.route[(size_t)f].route == STAGED) B.n_staged++;
    }
    B.img_pitch = align_up(B.img, 256);                      // (ingest_kernel reads 16-byte aligned sources)
    L.h_img = take(B.n_staged * B.img_pitch);
    L.h_total = o;
    o = 0;
    L.g_run = take(L.run_bytes); L.g_map = take(L.map_bytes); L.g_pw = take(C * 24); L.g_cell = take(C * 4); L.g_px0 = take(C * 16);
    L.g_px = take(C * 16); L.g_ck = take(C * 4); L.g_cf = take(C * 4); L.g_rpx = take(C * 8); L.g_rl = take(C * 4); L.g_rb = take(C * 24);
    L.g_ib = take(C); L.g_sl = take(C * 4); L.g_cv = take(C); L.g_grid = take(C); L.g_pob = take(NF * MM * 24);
    L.g_pow = take(NF * MM * 24); L.g_pol = take(NF * MM * 4); L.g_pou = take(NF * MM); L.g_pon = take(NF * 4); L.g_Topt = take(NF * 96);
    L.g_total = o;
    if (int rc = ensure_stage(ctx, L.h_total > L.g_total ? L.h_total : L.g_total)) return rc;
    B.h = (uint8_t*)ctx->h_pinned;
    B.g = (uint8_t*)ctx->d_stage;
    return pinned_device_ptr(ctx, &B.hd);
}

// Run's range: features, poses seeded (src/Tracking.cpp:201), counts and statistics cleared
static void tracks_pack_run(TrackBatch& B) {
    const TrackLayout& L = B.L;
    uint8_t* const h = B.h;
    const size_t NF = (size_t)B.n, MF = B.MF;
    for (int s = 0; s < B.n; ++s) {
        const dsdtm_track_desc* d = &B.descs[B.order[(size_t)s]];
        const size_t nf = (size_t)d->n_ref_features, S = (size_t)s;
        if (nf) {
            memcpy(h + L.h_px + S * MF * 8, d->ref_px_xy, nf * 8); memcpy(h + L.h_bear + S * MF * 24, d->ref_bearing, nf * 24);
            memcpy(h + L.h_pw + S * MF * 24, d->ref_p_world, nf * 24); memcpy(h + L.h_ini + S * MF, d->ref_initial, nf);
        }
        ((int32_t*)(h + L.h_nf))[s] = (int32_t)nf;
        memcpy(h + L.h_tr + S * 96, d->T_ref_w, 96);
        ((const uint8_t**)(h + L.h_rp))[s] = d->ref->d;
        if (B.resident) ((const uint8_t**)(h + L.h_cp))[s] = B.cur[(size_t)B.order[S]]->d;
        memcpy(h + L.h_T + S * 96, d->T_seed, 96);
    }
    memset(h + L.h_nt, 0, NF * 4);
    memset(h + L.h_st, 0, NF * sizeof(dsdtm_align_stats));
}

// the new frames: level 0 of each into its slot of the slab — the first slot's ingest also moves Run's range (a first slot that
// travels by the copy engine gets an ingest launch with no image for it) —, then the pyramids. Resident: Run's range only.
static int tracks_ingest(dsdtm_ctx* ctx, TrackBatch& B, hipStream_t stream) {
    const TrackLayout& L = B.L;
    const RunRange run_range = {B.hd + L.h_run, B.g + L.g_run, L.run_bytes};
    if (B.resident) { HIP_TRY(ctx, ingest_launch(nullptr, nullptr, 0, run_range.src, run_range.dst, run_range.bytes, stream)); return DSDTM_OK; }
    size_t staged = 0;
    for (int s = 0; s < B.n; ++s) {
        const int f = B.order[(size_t)s];
        const dsdtm_track_desc* d = &B.descs[f];
        ImageRoute r = B.route[(size_t)f];
        if (r.route == STAGED) {
            copy_rows(B.h + L.h_img + staged * B.img_pitch, (size_t)d->width, d->image, (size_t)d->stride, (size_t)d->width, (size_t)d->height);
            r.dev = B.hd + L.h_img + staged * B.img_pitch;
            staged++;
        }
        if (int rc = enqueue_level0(ctx, r, d->image, d->width, d->height, d->stride, B.slab + (size_t)s * B.pitch, s == 0 ? &run_range : nullptr, stream)) return rc;
    }
    const TrackPlan& P = B.plans[0];
    return dsdtm_pyrdown_batch_device(ctx, B.slab, B.pitch, B.n, P.pl.levels, P.pl.w, P.pl.h, P.st, P.pl.off, stream);
}

// Run: one launch per register band present, one-CU kernels, reference pyramids through the pointer table
static int tracks_run_bands(dsdtm_ctx* ctx, TrackBatch& B, hipStream_t stream) {
    const TrackLayout& L = B.L;
    const size_t MF = B.MF;
    uint8_t* const gr = B.g + L.g_run - L.h_run;      // device address of pinned offset X inside Run's range: gr + X
    for (int b = 0; b < 6; ++b) {
        const int cnt = B.band_lo[b + 1] - B.band_lo[b];
        if (cnt <= 0) continue;
        const size_t S = (size_t)B.band_lo[b];
        dsdtm_batch_desc bd;
        memset(&bd, 0, sizeof bd);
        bd.n_pairs = cnt; bd.max_features = (int)MF;
        fill_levels(bd, B.plans[0].pl);
        bd.pyr_pitch = B.pitch;
        bd.ref_pyr = B.resident ? B.cur[(size_t)B.order[S]]->d : B.slab + S * B.pitch;   // (not read by the pointer-table kernel: a range of the right size)
        bd.cur_pyr = bd.ref_pyr;                                  // (resident: not read either — every pair goes through cur_ptrs)
        bd.px_xy = (const float*)(gr + L.h_px) + S * MF * 2; bd.bearing = (const double*)(gr + L.h_bear) + S * MF * 3;
        bd.p_world = (const double*)(gr + L.h_pw) + S * MF * 3; bd.initial = gr + L.h_ini + S * MF;
        bd.n_features = (const int32_t*)(gr + L.h_nf) + S;
        bd.T_ref_w = (const double*)(gr + L.h_tr) + S * 12; bd.T_cur_w = (double*)(gr + L.h_T) + S * 12;
        bd.n_tracked = (int32_t*)(gr + L.h_nt) + S; bd.stats = (dsdtm_align_stats*)(gr + L.h_st) + S;
        LaunchMode mode;
        mode.single = true; mode.one_cu = true; mode.variant = (int)kBandVariant[b];
        mode.ref_ptrs = (const uint8_t* const*)(gr + L.h_rp) + S;
        if (B.resident) mode.cur_ptrs = (const uint8_t* const*)(gr + L.h_cp) + S;
        if (int rc = launch_batch(ctx, &bd, B.cam, &B.descs[0].align, stream, mode, nullptr)) return rc;
    }
    return DSDTM_OK;
}

// the local maps: packed in slot order (observations name keyframes in the concatenated table)
static void tracks_pack_maps(TrackBatch& B) {
    const TrackLayout& L = B.L;
    uint8_t* h = B.h;
    const uint8_t* gm = B.g + L.g_map - L.h_map;      // device address of pinned offset X inside the map range: gm + X
    const int n = B.n;
    size_t z = 0, kb = 0, mk = 0;
    int32_t* off = (int32_t*)(h + L.h_off);
    for (int s = 0; s < n; ++s) {
        const int f = B.order[(size_t)s];
        const dsdtm_track_desc* d = &B.descs[f];
        const size_t M = (size_t)d->n_points, c0 = (size_t)B.col0[(size_t)s], nnz = (size_t)B.plans[(size_t)f].nnz;
        const size_t cols = (s + 1 < n ? (size_t)B.col0[(size_t)s + 1] : B.C) - c0;
        ((int32_t*)(h + L.h_c0))[s] = (int32_t)c0;
        ((int32_t*)(h + L.h_np))[s] = (int32_t)M;
        if (d->mask) {
            copy_rows(h + L.h_mask + mk * B.img, (size_t)d->width, d->mask, (size_t)d->mask_stride, (size_t)d->width, (size_t)d->height);
            ((const uint8_t**)(h + L.h_fmask))[s] = gm + L.h_mask + mk * B.img;
            mk++;
        } else ((const uint8_t**)(h + L.h_fmask))[s] = nullptr;
        if (M) { memcpy(h + L.h_mpw + c0 * 24, d->mp_world, M * 24); memcpy(h + L.h_found + c0 * 4, d->mp_found, M * 4); memcpy(h + L.h_bad + c0, d->mp_bad, M); }
        for (size_t i = 0; i < cols; ++i) off[c0 + i] = (int32_t)(z + (i < M ? (size_t)d->obs_offset[i] : nnz));
        if (nnz) {
            for (size_t j = 0; j < nnz; ++j) ((int32_t*)(h + L.h_okf))[z + j] = d->obs_kf[j] + (int32_t)kb;
            memcpy(h + L.h_opx + z * 8, d->obs_px, nnz * 8); memcpy(h + L.h_olv + z * 4, d->obs_level, nnz * 4); memcpy(h + L.h_ob + z * 24, d->obs_bearing, nnz * 24);
        }
        if (d->n_kf > 0) memcpy(h + L.h_Tkf + kb * 96, d->T_kf_w, (size_t)d->n_kf * 96);
        for (int k = 0; k < d->n_kf; ++k) ((const uint8_t**)(h + L.h_kfp))[kb + (size_t)k] = d->kf[k]->d;
        z += nnz; kb += (size_t)d->n_kf;
    }
    off[B.C] = (int32_t)z;
    memcpy(h + L.h_bf, B.blk_frame.data(), B.NB * 4);
}

// the maps go up on a second stream while Run runs; reprojection + FindMatchDirect over all columns; the replays; the
// refinements; Run's outputs and the grid flags come back; the one wait
static int tracks_launch_and_wait(dsdtm_ctx* ctx, TrackBatch& B, bool want_grid, hipStream_t stream) {
    const TrackLayout& L = B.L;
    uint8_t *h = B.h, *g = B.g;
    const int n = B.n;
    if (!ctx->copy_stream[0]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream[0], hipStreamNonBlocking));
    HIP_TRY(ctx, hipMemcpyAsync(g + L.g_map, h + L.h_map, L.map_bytes, hipMemcpyHostToDevice, ctx->copy_stream[0]));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream[0]));
    TrackArgs t; WarpKernelArgs wa; A2DKernelArgs aa; PoseOptArgs pa;
    // (resident: aa.cur_pyr is not read — the workgroups go through t.cur_ptrs)
    bind_track_kernels(L, g, B.hd, B.cam, &B.descs[0], B.plans[0], n, (int)B.C, (int)B.NK, B.resident ? B.cur[(size_t)B.order[0]]->d : B.slab,
                       B.pitch, t, wa, aa, pa);
    const uint8_t *gr = g + L.g_run - L.h_run, *gm = g + L.g_map - L.h_map;
    t.n_frames = n; t.blk_frame = (const int32_t*)(gm + L.h_bf); t.f_col0 = (const int32_t*)(gm + L.h_c0); t.f_np = (const int32_t*)(gm + L.h_np);
    t.f_mask = (const uint8_t* const*)(gm + L.h_fmask); t.in_grid = g + L.g_grid; t.max_points = B.max_points;
    t.cur_ptrs = B.resident ? (const uint8_t* const*)(gr + L.h_cp) : nullptr;
    t.run_out_n16 = 0;     // (n frames' Run results are too many for the match kernel's posted writes, the single call's way: one copy, below)
    memset(h + L.h_cnt, 0, (size_t)n * 16); memset(h + L.h_sm, 0, (size_t)n * sizeof(dsdtm_pose_opt_summary));
    HIP_TRY(ctx, track_match_launch(t, wa, aa, stream));
    HIP_TRY(ctx, track_replay_launch(t, stream));
    HIP_TRY(ctx, pose_opt_launch(pa, stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + L.h_T, g + L.g_run + (L.h_T - L.h_run), L.run_out_bytes, hipMemcpyDeviceToHost, stream));
    if (want_grid) HIP_TRY(ctx, hipMemcpyAsync(h + L.h_grid, g + L.g_grid, B.C, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    frames_settle(ctx);
    return DSDTM_OK;
}

// the frames (all or nothing; resident: the caller's own, untouched) and every frame's results, in the caller's order
static int tracks_frames_and_readback(dsdtm_ctx* ctx, TrackBatch& B, size_t slab_bytes, dsdtm_track_result* results, dsdtm_track_match* matches,
                                      double* residual_norm, uint8_t* in_grid) {
    const int n = B.n; const size_t NF = (size_t)n;
    const bool resident = B.resident;
    FrameSlab* sl = resident ? nullptr : new (std::nothrow) FrameSlab();
    std::vector<dsdtm_frame*> fr;
    std::vector<size_t> grid_start;
    bool ok = resident || sl != nullptr;
    if (ok) { try { fr.assign(NF, nullptr); grid_start.assign(NF, 0); } catch (...) { ok = false; } }
    for (int s = 0; ok && !resident && s < n; ++s) {
        dsdtm_frame* f = new (std::nothrow) dsdtm_frame();
        if (!f) { ok = false; break; }
        f->owner = ctx; f->device = ctx->device; f->d = B.slab + (size_t)s * B.pitch; f->pitch = B.pitch; f->pl = B.plans[0].pl; f->slab = sl;
        fr[(size_t)s] = f;
    }
    if (!ok) {
        for (dsdtm_frame* f : fr) delete f;
        delete sl;
        set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM;
    }
    if (sl) { sl->owner = ctx; sl->device = ctx->device; sl->d = B.slab; sl->bytes = slab_bytes; sl->refs.store(n); }
    size_t grid_at = 0;
    for (int f = 0; f < n; ++f) { grid_start[(size_t)f] = grid_at; grid_at += (size_t)B.descs[f].n_points; }
    for (int s = 0; s < n; ++s) {
        const int f = B.order[(size_t)s];
        dsdtm_track_result* res = &results[f];
        if (!resident) res->frame = fr[(size_t)s];
        (void)read_track_result(B.h, B.L, (size_t)s, B.MM, B.descs[0].min_tracked, res, matches + (size_t)f * B.MM, residual_norm + (size_t)f * B.MM);   // (settled: checked by the caller)
        if (in_grid && B.descs[f].n_points > 0) memcpy(in_grid + grid_start[(size_t)f], B.h + B.L.h_grid + (size_t)B.col0[(size_t)s], (size_t)B.descs[f].n_points);
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_track_frames(dsdtm_ctx* ctx, const dsdtm_camera* cam, int n_frames, const dsdtm_track_desc* descs,
                                  dsdtm_track_result* results, dsdtm_track_match* matches, double* residual_norm, uint8_t* in_grid) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n_frames < 0 || n_frames > DSDTM_TRACK_FRAMES_MAX) { set_err(ctx, "track_frames: n_frames %d outside 0..%d", n_frames, DSDTM_TRACK_FRAMES_MAX); return DSDTM_ERR_INVALID; }
    if (n_frames == 0) return DSDTM_OK;
    if (!cam || !descs || !results || !matches || !residual_norm) { set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID; }
    const int n = n_frames;
    const bool resident = descs[0].image == nullptr;               // all or none: frame 0 decides, every other frame must agree
    // (checked before `results` is touched: in a mixture some results[f].frame are the caller's frames, and stay so)
    for (int f = 0; f < n; ++f)
        if ((descs[f].image == nullptr) != resident) {
            set_err(ctx, "track_frames: frame %d: image is %s, frame 0's is %s (a call runs on resident frames — image NULL, results[f].frame set — for all of its frames or for none)",
                    f, descs[f].image ? "set" : "NULL", resident ? "NULL" : "set");
            return DSDTM_ERR_INVALID;
        }
    TrackBatch B;
    B.n = n; B.resident = resident; B.cam = cam; B.descs = descs; B.slab = nullptr;
    if (resident) {
        try { B.cur.resize((size_t)n); } catch (...) { set_err(ctx, "out of host memory"); return DSDTM_ERR_NOMEM; }
        for (int f = 0; f < n; ++f) B.cur[(size_t)f] = results[f].frame;
    }
    for (int f = 0; f < n; ++f) {
        memset(&results[f], 0, sizeof results[f]);
        if (resident) results[f].frame = B.cur[(size_t)f];         // in/out: the caller's before, during and after the call
    }
    if (int rc = tracks_check(ctx, B)) return rc;
    if (int rc = tracks_order_and_sizes(ctx, B)) return rc;
    if (int rc = tracks_layout(ctx, B)) return rc;
    hipStream_t stream = ctx->stream;
    // the slab (resident mode: none — the frames are where they are)
    const size_t slab_bytes = B.pitch * (size_t)n;
    unsigned long long frames_seq = 0;          // the latest prefetch number among the pooled slab, the current (resident), reference and key frames
    uint8_t*& slab = B.slab;
    slab = resident ? nullptr : pool_take(ctx, slab_bytes, &frames_seq);
    const unsigned long long slab_seq = frames_seq;   // (a pooled buffer whose prefetch may still be writing it: it goes back with this number)
    for (int f = 0; f < n; ++f) if (B.plans[(size_t)f].frames_seq > frames_seq) frames_seq = B.plans[(size_t)f].frames_seq;
    if (resident) HIP_TRY(ctx, hipSetDevice(ctx->device));
    else if (!slab && (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void**)&slab, slab_bytes) != hipSuccess)) {
        (void)hipGetLastError();
        set_err(ctx, "hipMalloc of a %zu-byte slab of %d frames failed", slab_bytes, n);
        return DSDTM_ERR_NOMEM;
    }
    auto fail = [&](int rc) {
        if (ctx->copy_stream[0]) (void)hipStreamSynchronize(ctx->copy_stream[0]);
        (void)hipStreamSynchronize(stream);
        if (slab && !pool_give(ctx, ctx, ctx->device, slab, slab_bytes, slab_seq)) (void)hipFree(slab);
        return rc;
    };
    if (int rc = frames_consume(ctx, frames_seq, stream)) return fail(rc);
    tracks_pack_run(B);
    if (int rc = tracks_ingest(ctx, B, stream)) return fail(rc);
    volatile unsigned* h_flag = ctx->h_flags + dsdtm_ctx::FLAG_SINGLE;
    *h_flag = 0;
    if (int rc = tracks_run_bands(ctx, B, stream)) return fail(rc);
    tracks_pack_maps(B);
    if (int rc = tracks_launch_and_wait(ctx, B, in_grid != nullptr, stream)) return fail(rc);
    if (*h_flag) {
        *h_flag = 0;
        clear_stream_counters(ctx, ctx->stream);
        set_err(ctx, "sparse-align kernel: intra-workgroup hand-over timed out"); return fail(DSDTM_ERR_HIP);
    }
    const int32_t* cnt = (const int32_t*)(B.h + B.L.h_cnt);
    for (int s = 0; s < n; ++s) {
        const bool lost = ((const int32_t*)(B.h + B.L.h_nt))[s] < descs[0].min_tracked;
        if (cnt[4 * s + 2] == 2 && !lost) { set_err(ctx, "track_frames: frame %d: the replay of the cell walk did not settle", B.order[(size_t)s]); return fail(DSDTM_ERR_HIP); }
    }
    const int rc = tracks_frames_and_readback(ctx, B, slab_bytes, results, matches, residual_norm, in_grid);
    return rc ? fail(rc) : DSDTM_OK;
}
