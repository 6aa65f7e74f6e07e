// api_local_ba.cpp — dsdtm_local_ba / dsdtm_local_ba_batch_device of include/dsdtm_amd.h: the checks, the descriptors and the
// workspace of the local-BA launches (local_ba.hip). The fake-HIP sanitizer programs under tests/ do not list this file.
#include <cmath>
#include <cstring>

#include "api_internal.h"

using namespace dsdtm;
using namespace dsdtm::detail;

// ---- Optimizer::LocalBundleAdjustment ----------------------------------------------------------------------------------
static const char* lba_check_reason(int mask) {
    if (mask & LBA_CHECK_KF_INDEX) return "keyframe index out of range";
    if (mask & LBA_CHECK_POINT_INDEX) return "point index out of range";
    if (mask & LBA_CHECK_LEVEL) return "level out of range";
    if (mask & LBA_CHECK_ORDER) return "point index decreases";
    if (mask & LBA_CHECK_DUPLICATE) return "a keyframe observes a point twice";
    if (mask & LBA_CHECK_NO_FREE) return "no free keyframe";
    if (mask & LBA_CHECK_FREE_LIMIT) return "free keyframes over the limit of 16";
    return "constant keyframes over the limit of 64";
}
static int lba_check_counts(dsdtm_ctx* ctx, int i, const dsdtm_local_ba_problem& q) {
    const char* what = nullptr;
    // (the release library holds no DSDTM_* string: the limits are named by their values)
    int limit = 0;
    if (q.n_keyframes <= 0) what = "no keyframe (at least one free keyframe is needed)";
    else if (q.n_keyframes > DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF)
        what = "keyframes over the limit of free + constant keyframes", limit = DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF;
    else if (q.n_points < 0 || q.n_points > DSDTM_LBA_MAX_POINTS) what = "points outside 0 .. the point limit", limit = DSDTM_LBA_MAX_POINTS;
    else if (q.n_observations < 0 || q.n_observations > DSDTM_LBA_MAX_OBSERVATIONS)
        what = "observations outside 0 .. the observation limit", limit = DSDTM_LBA_MAX_OBSERVATIONS;
    else if (q.keyframe_offset < 0 || q.point_offset < 0 || q.observation_offset < 0) what = "negative offset";
    if (!what) return DSDTM_OK;
    set_err(ctx, "local_ba: problem %d: %s (%d)", i, what, limit);
    return DSDTM_ERR_INVALID;
}

extern "C" int dsdtm_local_ba_batch_device(dsdtm_ctx* ctx, int n_problems, const dsdtm_local_ba_problem* problems,
                                           double* T_c2w, const uint8_t* kf_constant, double* points,
                                           const int32_t* obs_kf, const int32_t* obs_point, const double* obs_bearing,
                                           const int32_t* obs_level, const dsdtm_local_ba_params* params,
                                           uint8_t* outlier, dsdtm_local_ba_summary* summary, void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n_problems < 0 || !params || params->max_iterations < 0 || !(params->delta >= 0.0) || !std::isfinite(params->delta)) {
        set_err(ctx, "local_ba: bad argument"); return DSDTM_ERR_INVALID;
    }
    if (n_problems == 0) return DSDTM_OK;
    if (!problems || !T_c2w || !kf_constant || !points || !obs_kf || !obs_point || !obs_bearing || !obs_level || !outlier || !summary) {
        set_err(ctx, "local_ba: NULL argument"); return DSDTM_ERR_INVALID;
    }
    // every problem is checked before the solve is enqueued: one bad problem and no problem runs, nothing is written
    std::vector<LocalBaProblemDev> dev((size_t)n_problems);
    size_t ws = 0;
    for (int i = 0; i < n_problems; ++i) {
        const dsdtm_local_ba_problem& q = problems[i];
        if (int rc = lba_check_counts(ctx, i, q)) return rc;
        LocalBaProblemDev& d = dev[(size_t)i];
        d.n_kf = q.n_keyframes; d.n_pts = q.n_points; d.n_obs = q.n_observations; d.reserved = 0;
        d.kf_off = q.keyframe_offset; d.pt_off = q.point_offset; d.obs_off = q.observation_offset;
        d.ws_off = (int64_t)ws;
        ws += local_ba_workspace_bytes(q.n_points, q.n_observations);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->lba_event) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->lba_event, hipEventDisableTiming));
    if (ctx->lba_recorded) HIP_TRY(ctx, hipEventSynchronize(ctx->lba_event));    // the previous launch is done with the buffers
    const size_t desc_bytes = align_up(dev.size() * sizeof(LocalBaProblemDev), 256);
    const size_t check_bytes = align_up(dev.size() * sizeof(int32_t), 256);
    const size_t dev_bytes = desc_bytes + check_bytes + ws, host_bytes = desc_bytes + check_bytes;
    if (dev_bytes > ctx->lba_cap) {
        if (ctx->d_lba) (void)hipFree(ctx->d_lba);
        ctx->d_lba = nullptr; ctx->lba_cap = 0;
        const size_t cap = align_up(dev_bytes + dev_bytes / 4, 1 << 16);
        HIP_TRY(ctx, hipMalloc(&ctx->d_lba, cap));
        ctx->lba_cap = cap;
    }
    if (host_bytes > ctx->h_lba_cap) {
        if (ctx->h_lba) (void)hipHostFree(ctx->h_lba);
        ctx->h_lba = nullptr; ctx->h_lba_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->h_lba, host_bytes, hipHostMallocDefault));
        ctx->h_lba_cap = host_bytes;
    }
    memcpy(ctx->h_lba, dev.data(), dev.size() * sizeof(LocalBaProblemDev));
    const hipStream_t stream = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lba, ctx->h_lba, dev.size() * sizeof(LocalBaProblemDev), hipMemcpyHostToDevice, stream));
    LocalBaArgs a;
    a.n_problems = n_problems; a.max_iterations = params->max_iterations; a.delta = params->delta;
    a.problems = (const LocalBaProblemDev*)ctx->d_lba;
    a.T = T_c2w; a.kf_const = kf_constant; a.points = points;
    a.obs_kf = obs_kf; a.obs_pt = obs_point; a.bearing = obs_bearing; a.level = obs_level;
    a.outlier = outlier; a.summary = summary;
    a.check = (int32_t*)((uint8_t*)ctx->d_lba + desc_bytes);
    a.ws = (uint8_t*)ctx->d_lba + desc_bytes + check_bytes;
    // the checks of the device arrays (indices, levels, order, constant flags): a read-only kernel whose masks are read back
    // here — the call waits until the stream has reached them; the solve itself stays asynchronous
    HIP_TRY(ctx, local_ba_check_launch(a, stream));
    int32_t* h_check = (int32_t*)((uint8_t*)ctx->h_lba + desc_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(h_check, a.check, dev.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->lba_event, stream));
    ctx->lba_recorded = true;
    HIP_TRY(ctx, hipEventSynchronize(ctx->lba_event));
    for (int i = 0; i < n_problems; ++i)
        if (h_check[i]) { set_err(ctx, "local_ba: problem %d: %s", i, lba_check_reason(h_check[i])); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, local_ba_launch(a, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->lba_event, stream));
    ctx->lba_recorded = true;
    return DSDTM_OK;
}

extern "C" int dsdtm_local_ba(dsdtm_ctx* ctx, int n_keyframes, double* T_c2w, const uint8_t* kf_constant,
                              int n_points, double* points, int n_observations, const int32_t* obs_kf, const int32_t* obs_point,
                              const double* obs_bearing, const int32_t* obs_level, const dsdtm_local_ba_params* params,
                              uint8_t* outlier, dsdtm_local_ba_summary* summary) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!params || params->max_iterations < 0 || !(params->delta >= 0.0) || !std::isfinite(params->delta)) {
        set_err(ctx, "local_ba: bad argument"); return DSDTM_ERR_INVALID;
    }
    dsdtm_local_ba_problem q = {n_keyframes, n_points, n_observations, 0, 0, 0, 0};
    if (int rc = lba_check_counts(ctx, 0, q)) return rc;
    if (!T_c2w || !kf_constant || !summary || (n_points > 0 && !points) ||
        (n_observations > 0 && (!obs_kf || !obs_point || !obs_bearing || !obs_level || !outlier))) {
        set_err(ctx, "local_ba: NULL argument"); return DSDTM_ERR_INVALID;
    }
    int n_free = 0;
    for (int k = 0; k < n_keyframes; ++k) n_free += kf_constant[k] ? 0 : 1;
    if (n_free == 0) { set_err(ctx, "local_ba: no free keyframe"); return DSDTM_ERR_INVALID; }
    if (n_free > DSDTM_LBA_MAX_FREE_KF) {
        set_err(ctx, "local_ba: %d free keyframes over the limit of %d", n_free, DSDTM_LBA_MAX_FREE_KF); return DSDTM_ERR_INVALID;
    }
    if (n_keyframes - n_free > DSDTM_LBA_MAX_CONST_KF) {
        set_err(ctx, "local_ba: %d constant keyframes over the limit of %d", n_keyframes - n_free, DSDTM_LBA_MAX_CONST_KF);
        return DSDTM_ERR_INVALID;
    }
    for (int i = 0; i < n_observations; ++i) {
        const int k = obs_kf[i], p = obs_point[i], l = obs_level[i];
        if (k < 0 || k >= n_keyframes) { set_err(ctx, "local_ba: observation %d: keyframe index %d out of range", i, k); return DSDTM_ERR_INVALID; }
        if (p < 0 || p >= n_points) { set_err(ctx, "local_ba: observation %d: point index %d out of range", i, p); return DSDTM_ERR_INVALID; }
        if (l < 0 || l >= DSDTM_MAX_LEVELS) { set_err(ctx, "local_ba: observation %d: level %d out of range", i, l); return DSDTM_ERR_INVALID; }
        if (i > 0 && obs_point[i - 1] > p) { set_err(ctx, "local_ba: observation %d: point index decreases", i); return DSDTM_ERR_INVALID; }
        for (int j = i - 1; j >= 0 && obs_point[j] == p; --j)
            if (obs_kf[j] == k) { set_err(ctx, "local_ba: observation %d: keyframe %d observes point %d twice", i, k, p); return DSDTM_ERR_INVALID; }
    }
    const size_t K = (size_t)n_keyframes, NP = (size_t)n_points, N = (size_t)n_observations;
    size_t o = 0;
    const size_t o_T = o;   o += align_up(K * 96, 256);        // in/out
    const size_t o_X = o;   o += align_up(NP * 24, 256);       // in/out
    const size_t o_out = o; o += align_up(N, 256);             // out
    const size_t o_sm = o;  o += align_up(sizeof(dsdtm_local_ba_summary), 256);   // out
    const size_t out_end = o;
    const size_t o_c = o;   o += align_up(K, 256);
    const size_t o_k = o;   o += align_up(N * 4, 256);
    const size_t o_p = o;   o += align_up(N * 4, 256);
    const size_t o_b = o;   o += align_up(N * 24, 256);
    const size_t o_l = o;   o += align_up(N * 4, 256);
    const size_t total = o;
    if (int rc = ensure_stage(ctx, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    memcpy(h + o_T, T_c2w, K * 96);
    if (NP) memcpy(h + o_X, points, NP * 24);
    memcpy(h + o_c, kf_constant, K);
    if (N) {
        memcpy(h + o_k, obs_kf, N * 4);
        memcpy(h + o_p, obs_point, N * 4);
        memcpy(h + o_b, obs_bearing, N * 24);
        memcpy(h + o_l, obs_level, N * 4);
    }
    HIP_TRY(ctx, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = dsdtm_local_ba_batch_device(ctx, 1, &q, (double*)(d + o_T), d + o_c, (double*)(d + o_X),
                                             (const int32_t*)(d + o_k), (const int32_t*)(d + o_p), (const double*)(d + o_b),
                                             (const int32_t*)(d + o_l), params, d + o_out,
                                             (dsdtm_local_ba_summary*)(d + o_sm), ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h, d, out_end, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T_c2w, h + o_T, K * 96);
    if (NP) memcpy(points, h + o_X, NP * 24);
    if (N) memcpy(outlier, h + o_out, N);
    memcpy(summary, h + o_sm, sizeof(*summary));
    return DSDTM_OK;
}
