// slam_api.cpp — the C ABI of include/dsdtm_amd_slam.h (libdsdtm_amd_slam.so). The resident map and its entries are the ONE
// implementation of trackmap_api_body.h and the mapping thread's three entries the ONE implementation of mapping_api_body.h, both
// compiled here under the dsdtm_slam_* names; behind them the checks and the packing of dsdtm_slam_track_commit: one upload (the maps
// and the descs as the device sees them, the matches), the two launches of aftertrack.hip, one read-back, one wait. There is no CPU
// compute path here (the host evaluation is host/dsdtm_slam_host.hpp, which needs no library).
#define TM_API(name) dsdtm_slam_##name
#define TM_CTX dsdtm_slam_ctx
#define TM_LIB "dsdtm_amd_slam"
#define MP_API(name) dsdtm_slam_##name
#include "aftertrack.h"
#include "trackmap_api_body.h"
#include "mapping_api_body.h"

extern "C" int dsdtm_slam_track_commit(dsdtm_slam_ctx* ctx, double outlier_threshold, int n, const dsdtm_slam_commit_desc* descs, int bad_capacity,
                                       int32_t* bad_points, dsdtm_slam_commit_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_LOCALMAP_MAX_DESCS) { set_err(ctx, "track_commit: n = %d outside 0..%d", n, DSDTM_LOCALMAP_MAX_DESCS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!std::isfinite(outlier_threshold)) { set_err(ctx, "track_commit: outlier_threshold is not finite"); return DSDTM_ERR_INVALID; }
    if (bad_capacity < 0) { set_err(ctx, "track_commit: bad_capacity = %d is negative", bad_capacity); return DSDTM_ERR_INVALID; }
    const char* null_arg = !descs ? "descs" : !results ? "results" : bad_capacity > 0 && !bad_points ? "bad_points" : nullptr;
    if (null_arg) { set_err(ctx, "track_commit: %s is NULL", null_arg); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the distinct maps on the way, each with its descs in desc order
    const size_t N = (size_t)n;
    std::vector<dsdtm_trackmap*> maps;
    std::vector<std::vector<int32_t>> descs_of;
    std::vector<int32_t> sorted;
    for (int t = 0; t < n; ++t) {
        const dsdtm_slam_commit_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (!owns(ctx, d.map)) bad = "map is not a map of this context";
        else if (d.n_matches < 0 || d.n_matches > DSDTM_SLAM_MAX_MATCHES) bad = "n_matches out of range";
        else if (d.n_matches > 0 && !d.point) bad = "point is NULL";
        else if (d.n_matches > 0 && !d.residual_norm) bad = "residual_norm is NULL";
        if (bad) { set_err(ctx, "track_commit: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        for (int i = 0; i < d.n_matches; ++i)
            if (d.point[i] < 0 || (int64_t)d.point[i] >= d.map->used[0]) {
                set_err(ctx, "track_commit: desc %d: point[%d] = %d is not below the map's %lld points", t, i, d.point[i], (long long)d.map->used[0]);
                return DSDTM_ERR_INVALID;
            }
        sorted.assign(d.point, d.point + d.n_matches);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) { set_err(ctx, "track_commit: desc %d: point %d occurs twice", t, *dup); return DSDTM_ERR_INVALID; }
        const size_t m = std::find(maps.begin(), maps.end(), d.map) - maps.begin();
        if (m == maps.size()) { maps.push_back(d.map); descs_of.emplace_back(); }
        descs_of[m].push_back(t);
    }
    // the block's layout: AtMapDev x M | AtDescDev x n | the maps' desc lists, the matches | outputs | temporaries
    const size_t M = maps.size();
    std::vector<AtMapDev> mrec(M);
    std::vector<AtDescDev> drec(N);
    const size_t descs_off = align_up(M * sizeof(AtMapDev), 16);
    Taker take{align_up(descs_off + N * sizeof(AtDescDev), 16)};
    long long max_S = 0;
    for (size_t m = 0; m < M; ++m) {
        AtMapDev& r = mrec[m];
        memset(&r, 0, sizeof r);
        r.points = maps[m]->d_points; r.found = maps[m]->d_found; r.slots = maps[m]->d_slots; r.obs = maps[m]->d_obs;
        r.S = maps[m]->used[2]; r.P = (int32_t)maps[m]->used[0]; r.n_descs = (int32_t)descs_of[m].size();
        r.desc_list = take(descs_of[m].size() * 4);
        max_S = std::max(max_S, (long long)r.S);
    }
    for (int t = 0; t < n; ++t) {
        AtDescDev& r = drec[(size_t)t];
        memset(&r, 0, sizeof r);
        r.n_matches = descs[t].n_matches; r.bad_cap = std::min(bad_capacity, descs[t].n_matches);
        r.point = take((size_t)r.n_matches * 4); r.norm = take((size_t)r.n_matches * 8);
    }
    const size_t up = align_up(take.o, 16);
    take.o = up;
    for (AtDescDev& r : drec) { r.result = take(sizeof(dsdtm_slam_commit_result)); r.found_after = take((size_t)r.n_matches * 4); r.bad_list = take((size_t)r.bad_cap * 4); }
    const size_t back = align_up(take.o, 256);
    take.o = back;
    for (size_t m = 0; m < M; ++m) { mrec[m].stamp = take((size_t)mrec[m].P); mrec[m].n_new_bad = take(4); }
    if (take.o > (size_t)DSDTM_TRACKMAP_MAX_CALL_BYTES) {
        set_err(ctx, "track_commit: the call's block for %d descs on %zu maps exceeds %lld bytes (one per point of every distinct map)", n, M, (long long)DSDTM_TRACKMAP_MAX_CALL_BYTES);
        return DSDTM_ERR_INVALID;
    }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, take.o)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, mrec.data(), M * sizeof(AtMapDev));
    memcpy(h + descs_off, drec.data(), N * sizeof(AtDescDev));
    for (size_t m = 0; m < M; ++m) memcpy(h + mrec[m].desc_list, descs_of[m].data(), descs_of[m].size() * 4);
    for (int t = 0; t < n; ++t) {
        const AtDescDev& r = drec[(size_t)t];
        if (!r.n_matches) continue;
        memcpy(h + r.point, descs[t].point, (size_t)r.n_matches * 4);
        memcpy(h + r.norm, descs[t].residual_norm, (size_t)r.n_matches * 8);
    }
    AtCommitArgs a;
    memset(&a, 0, sizeof a);
    a.block = g; a.descs = descs_off; a.n_maps = (int)M; a.n = n; a.max_S = max_S; a.threshold = outlier_threshold;
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(aftertrack_commit_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + up, g + up, back - up, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    for (int t = 0; t < n; ++t) {
        const AtDescDev& r = drec[(size_t)t];
        dsdtm_slam_commit_result res;
        memcpy(&res, h + r.result, sizeof res);
        res.overflow_bad = res.n_bad > bad_capacity ? 1 : 0; res.reserved = 0;
        const size_t m = (size_t)std::min(std::max(res.n_bad, 0), r.bad_cap);
        if (m) memcpy(bad_points + (size_t)t * (size_t)bad_capacity, h + r.bad_list, m * 4);
        if (descs[t].found_after && r.n_matches) memcpy(descs[t].found_after, h + r.found_after, (size_t)r.n_matches * 4);
        results[t] = res;
    }
    return DSDTM_OK;
}

// One upload (the trackers' records with the offsets of their arrays, the gather records, the index lists), the gather launch of
// aftertrack.hip, the decision launch of keyframe.hip, one read-back of n verdicts, one wait. The block's layout:
// KeyframeTrackerDev x n (the blob keyframe.hip takes) | AtGatherDev x n | the index lists | verdicts | the gathered arrays.
extern "C" int dsdtm_slam_need_keyframes(dsdtm_slam_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* prm, int n,
                                         const dsdtm_slam_keyframe_desc* descs, dsdtm_keyframe_verdict* verdicts) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam) { set_err(ctx, "need_keyframes: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!prm) { set_err(ctx, "need_keyframes: params is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_LOCALMAP_MAX_DESCS) { set_err(ctx, "need_keyframes: n = %d outside 0..%d", n, DSDTM_LOCALMAP_MAX_DESCS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (prm->px_samples < 1 || prm->px_samples > 64) { set_err(ctx, "need_keyframes: px_samples = %d outside 1..64", prm->px_samples); return DSDTM_ERR_INVALID; }
    if (!descs || !verdicts) { set_err(ctx, "need_keyframes: %s is NULL", !descs ? "descs" : "verdicts"); return DSDTM_ERR_INVALID; }
    const size_t N = (size_t)n;
    std::vector<KeyframeTrackerDev> rec(N);
    std::vector<AtGatherDev> grec(N);
    const size_t descs_off = align_up(N * sizeof(KeyframeTrackerDev), 16);
    Taker take{align_up(descs_off + N * sizeof(AtGatherDev), 16)};
    for (int t = 0; t < n; ++t) {
        const dsdtm_slam_keyframe_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (!owns(ctx, d.map)) bad = "map is not a map of this context";
        else if (!d.T_cur_w) bad = "T_cur_w is NULL";
        else if (d.n_cur_points < 0 || d.n_cur_points > DSDTM_KF_MAX_POINTS) bad = "n_cur_points out of range";
        else if (d.n_local_kf < 0 || d.n_local_kf > DSDTM_KF_MAX_LOCAL_KF) bad = "n_local_kf out of range";
        else if (d.n_cur_points > 0 && !d.cur_point) bad = "cur_point is NULL";
        else if (d.n_local_kf > 0 && !d.local_kf) bad = "local_kf is NULL";
        else if (d.kf < 0 || (int64_t)d.kf >= d.map->used[1]) bad = "kf is not a keyframe of the map";
        else if (!all_finite(d.T_cur_w, 12)) bad = "T_cur_w is not finite";
        if (bad) { set_err(ctx, "need_keyframes: tracker %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        for (int i = 0; i < d.n_cur_points; ++i)
            if (d.cur_point[i] < 0 || (int64_t)d.cur_point[i] >= d.map->used[0]) {
                set_err(ctx, "need_keyframes: tracker %d: cur_point[%d] = %d is not below the map's %lld points", t, i, d.cur_point[i], (long long)d.map->used[0]);
                return DSDTM_ERR_INVALID;
            }
        for (int i = 0; i < d.n_local_kf; ++i)
            if (d.local_kf[i] < 0 || (int64_t)d.local_kf[i] >= d.map->used[1]) {
                set_err(ctx, "need_keyframes: tracker %d: local_kf[%d] = %d is not below the map's %lld keyframes", t, i, d.local_kf[i], (long long)d.map->used[1]);
                return DSDTM_ERR_INVALID;
            }
        KeyframeTrackerDev& r = rec[(size_t)t];
        AtGatherDev& g = grec[(size_t)t];
        memset(&r, 0, sizeof r);
        memset(&g, 0, sizeof g);
        memcpy(r.T_cur, d.T_cur_w, 96);
        r.n_valid = d.n_valid; r.n_cur = d.n_cur_points; r.n_lkf = d.n_local_kf;      // (T_kf and n_kf: the gather)
        g.points = d.map->d_points; g.kfs = d.map->d_kfs; g.slots = d.map->d_slots;
        g.P = (int32_t)d.map->used[0]; g.K = (int32_t)d.map->used[1]; g.kf = d.kf;
        g.cur_point = take((size_t)d.n_cur_points * 4); g.local_kf = take((size_t)d.n_local_kf * 4);
    }
    const size_t up = align_up(take.o, 16), vbytes = N * sizeof(dsdtm_keyframe_verdict);
    take.o = up;
    const size_t v_off = (size_t)take(vbytes), back = align_up(take.o, 256);
    take.o = back;
    for (int t = 0; t < n; ++t) {
        KeyframeTrackerDev& r = rec[(size_t)t];
        const size_t nc = (size_t)r.n_cur, ns = (size_t)descs[t].map->kf_n_slots[(size_t)descs[t].kf], nl = (size_t)r.n_lkf;
        auto take16 = [&](size_t bytes) { take.o = align_up(take.o, 16); return take(bytes); };       // (the alignment dsdtm_need_keyframes gives them)
        r.cur_p = take16(nc * 24); r.cur_bad = take16(nc); r.kf_p = take16(ns * 24); r.kf_bad = take16(ns); r.lkf = take16(nl * 24);
    }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, take.o)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, rec.data(), N * sizeof(KeyframeTrackerDev));
    memcpy(h + descs_off, grec.data(), N * sizeof(AtGatherDev));
    for (int t = 0; t < n; ++t) {
        if (descs[t].n_cur_points) memcpy(h + grec[(size_t)t].cur_point, descs[t].cur_point, (size_t)descs[t].n_cur_points * 4);
        if (descs[t].n_local_kf) memcpy(h + grec[(size_t)t].local_kf, descs[t].local_kf, (size_t)descs[t].n_local_kf * 4);
    }
    AtGatherArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.block = g; ga.descs = descs_off; ga.n = n;
    KeyframeArgs a;
    memset(&a, 0, sizeof a);
    a.blob = g; a.verdict = (dsdtm_keyframe_verdict*)(g + v_off); a.n = n;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.prm = *prm;
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(aftertrack_gather_launch(ga, ctx->stream));
    API_TRY(need_keyframes_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + v_off, g + v_off, vbytes, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(verdicts, h + v_off, vbytes);
    stream_idle(ctx);
    return DSDTM_OK;
}
