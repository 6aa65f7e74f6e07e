// keyframe_api.cpp — the C ABI of include/dsdtm_amd_keyframe.h (libdsdtm_amd_keyframe.so): checks, packing, launch (the context: addon_host.h).
//
// The add-on's one entry packs the n trackers into one pinned blob, moves it with a single hipMemcpyAsync, launches
// keyframe.hip's kernel on the context's stream and copies the n verdicts back. There is no CPU compute path here (the host
// evaluation of the same rules is need_keyframe_host of host/dsdtm_host.hpp, which needs no library).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "keyframe.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_keyframe_ctx : dsdtm::AddonCtx {};      // (staging: the blob and the verdicts, at the same offsets on both sides)

extern "C" const char* dsdtm_keyframe_last_error(const dsdtm_keyframe_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_keyframe_create(int device, dsdtm_keyframe_ctx** out) { return addon_create("dsdtm_amd_keyframe", device, out); }
extern "C" void dsdtm_keyframe_destroy(dsdtm_keyframe_ctx* ctx) { addon_destroy(ctx); }

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// One upload (the trackers' records and arrays, packed into the pinned block), one launch, one read-back of n verdicts, one wait.
extern "C" int dsdtm_need_keyframes(dsdtm_keyframe_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* prm, int n,
                                    const dsdtm_keyframe_desc* descs, dsdtm_keyframe_verdict* verdicts) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam) { set_err(ctx, "need_keyframes: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!prm) { set_err(ctx, "need_keyframes: params is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_TRACK_FRAMES_MAX) { set_err(ctx, "need_keyframes: n = %d outside 0..%d", n, DSDTM_TRACK_FRAMES_MAX); return DSDTM_ERR_INVALID; }
    if (prm->px_samples < 1 || prm->px_samples > 64) { set_err(ctx, "need_keyframes: px_samples = %d outside 1..64", prm->px_samples); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs || !verdicts) { set_err(ctx, "need_keyframes: %s is NULL", !descs ? "descs" : "verdicts"); return DSDTM_ERR_INVALID; }
    // every tracker is checked before anything is enqueued; the blob's layout on the way
    const size_t N = (size_t)n;
    size_t o = align_up(N * sizeof(KeyframeTrackerDev), 16);
    std::vector<KeyframeTrackerDev> rec(N);
    for (int t = 0; t < n; ++t) {
        const dsdtm_keyframe_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.T_cur_w) bad = "T_cur_w is NULL";
        else if (!d.T_kf_w) bad = "T_kf_w is NULL";
        else if (d.n_cur_points < 0 || d.n_cur_points > DSDTM_KF_MAX_POINTS) bad = "n_cur_points out of range";
        else if (d.n_kf_points < 0 || d.n_kf_points > DSDTM_KF_MAX_POINTS) bad = "n_kf_points out of range";
        else if (d.n_local_kf < 0 || d.n_local_kf > DSDTM_KF_MAX_LOCAL_KF) bad = "n_local_kf out of range";
        else if (d.n_cur_points > 0 && !d.cur_p_world) bad = "cur_p_world is NULL";
        else if (d.n_kf_points > 0 && !d.kf_p_world) bad = "kf_p_world is NULL";
        else if (d.n_local_kf > 0 && !d.local_kf_centre) bad = "local_kf_centre is NULL";
        else if (!all_finite(d.T_cur_w, 12)) bad = "T_cur_w is not finite";
        else if (!all_finite(d.T_kf_w, 12)) bad = "T_kf_w is not finite";
        else if (!all_finite(d.cur_p_world, 3 * (size_t)d.n_cur_points)) bad = "cur_p_world is not finite";
        else if (!all_finite(d.kf_p_world, 3 * (size_t)d.n_kf_points)) bad = "kf_p_world is not finite";
        else if (!all_finite(d.local_kf_centre, 3 * (size_t)d.n_local_kf)) bad = "local_kf_centre is not finite";
        if (bad) { set_err(ctx, "need_keyframes: tracker %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        KeyframeTrackerDev& r = rec[(size_t)t];
        memcpy(r.T_cur, d.T_cur_w, 96); memcpy(r.T_kf, d.T_kf_w, 96);
        r.n_valid = d.n_valid; r.n_cur = d.n_cur_points; r.n_kf = d.n_kf_points; r.n_lkf = d.n_local_kf;
        r.cur_p = o; o += align_up((size_t)d.n_cur_points * 24, 16);
        r.cur_bad = o; o += align_up((size_t)d.n_cur_points, 16);
        r.kf_p = o; o += align_up((size_t)d.n_kf_points * 24, 16);
        r.kf_bad = o; o += align_up((size_t)d.n_kf_points, 16);
        r.lkf = o; o += align_up((size_t)d.n_local_kf * 24, 16);
    }
    const size_t blob = align_up(o, 256), vbytes = N * sizeof(dsdtm_keyframe_verdict);
    if (int rc = ensure_stage(ctx, blob + vbytes, blob + vbytes)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, rec.data(), N * sizeof(KeyframeTrackerDev));
    for (int t = 0; t < n; ++t) {
        const dsdtm_keyframe_desc& d = descs[t];
        const KeyframeTrackerDev& r = rec[(size_t)t];
        const size_t nc = (size_t)d.n_cur_points, nk = (size_t)d.n_kf_points, nl = (size_t)d.n_local_kf;
        if (nc) memcpy(h + r.cur_p, d.cur_p_world, nc * 24);
        if (nc) { if (d.cur_bad) memcpy(h + r.cur_bad, d.cur_bad, nc); else memset(h + r.cur_bad, 0, nc); }
        if (nk) memcpy(h + r.kf_p, d.kf_p_world, nk * 24);
        if (nk) { if (d.kf_bad) memcpy(h + r.kf_bad, d.kf_bad, nk); else memset(h + r.kf_bad, 0, nk); }
        if (nl) memcpy(h + r.lkf, d.local_kf_centre, nl * 24);
    }
    KeyframeArgs a;
    memset(&a, 0, sizeof a);
    a.blob = g; a.verdict = (dsdtm_keyframe_verdict*)(g + blob); a.n = n;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.prm = *prm;
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, o, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(need_keyframes_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + blob, g + blob, vbytes, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(verdicts, h + blob, vbytes);
    return DSDTM_OK;
}

extern "C" int dsdtm_need_keyframe(dsdtm_keyframe_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* prm,
                                   const dsdtm_keyframe_desc* desc, dsdtm_keyframe_verdict* verdict) {
    return dsdtm_need_keyframes(ctx, cam, prm, 1, desc, verdict);
}
