// homography_api.cpp — the C ABI of include/dsdtm_amd_homography.h (libdsdtm_amd_homography.so): checks, packing, launch (the context:
// addon_host.h).
//
// A call packs the n problems' records and correspondences into one pinned block, moves it with a single hipMemcpyAsync, launches
// homography.hip's kernel (one workgroup per problem) on the context's stream and reads the results and the masks back with one copy
// into the pinned block; the caller's arrays are written only after the wait succeeded. There is no CPU compute path here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "homography.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_homography_ctx : dsdtm::AddonCtx {};

extern "C" const char* dsdtm_homography_last_error(const dsdtm_homography_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_homography_create(int device, dsdtm_homography_ctx** out) { return addon_create("dsdtm_amd_homography", device, out); }
extern "C" void dsdtm_homography_destroy(dsdtm_homography_ctx* ctx) { addon_destroy(ctx); }

// what is wrong with one desc, or nullptr; `detail` receives the correspondence index where one is named
static const char* check_desc(const dsdtm_homography_desc& d, int* detail) {
    *detail = -1;
    if (d.m < 0 || d.m > DSDTM_HOMOGRAPHY_MAX_POINTS) return "m out of range";
    if (d.m > 0 && !d.points_a) return "points_a is NULL";
    if (d.m > 0 && !d.points_b) return "points_b is NULL";
    if (!std::isfinite(d.reproj_threshold)) return "reproj_threshold is not finite";
    if (!std::isfinite(d.confidence) || d.confidence >= 1.0) return "confidence is not below 1";
    if (d.max_hypotheses > DSDTM_HOMOGRAPHY_MAX_HYPOTHESES) return "max_hypotheses out of range";
    for (int i = 0; i < 2 * d.m; ++i) {
        if (!std::isfinite(d.points_a[i])) { *detail = i / 2; return "points_a is not finite at index"; }
        if (!std::isfinite(d.points_b[i])) { *detail = i / 2; return "points_b is not finite at index"; }
    }
    return nullptr;
}

extern "C" int dsdtm_find_homographies(dsdtm_homography_ctx* ctx, int n, const dsdtm_homography_desc* descs, dsdtm_homography_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_HOMOGRAPHY_MAX_PROBLEMS) { set_err(ctx, "find_homographies: n = %d outside 0..%d", n, DSDTM_HOMOGRAPHY_MAX_PROBLEMS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "find_homographies: descs is NULL"); return DSDTM_ERR_INVALID; }
    if (!results) { set_err(ctx, "find_homographies: results is NULL"); return DSDTM_ERR_INVALID; }
    {   // (the call allocates and waits: neither can be part of a capture)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) { set_err(ctx, "find_homographies: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    }
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   records | per problem: A, B (m x 2 floats each, 16-byte aligned) || results | per problem: mask (m bytes up to 16)
    const size_t N = (size_t)n;
    std::vector<size_t> a_at(N, 0), b_at(N, 0), mask_at(N, 0);
    size_t o = align_up(N * sizeof(HomographyDev), 256);
    for (int t = 0; t < n; ++t) {
        const dsdtm_homography_desc& d = descs[t];
        int detail = -1;
        if (const char* bad = check_desc(d, &detail)) {
            if (detail >= 0) set_err(ctx, "find_homographies: problem %d: %s %d", t, bad, detail);
            else set_err(ctx, "find_homographies: problem %d: %s", t, bad);
            return DSDTM_ERR_INVALID;
        }
        a_at[(size_t)t] = o; o += align_up((size_t)d.m * 8, 16);
        b_at[(size_t)t] = o; o += align_up((size_t)d.m * 8, 16);
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t out_begin = o;
    o += align_up(N * sizeof(dsdtm_homography_result), 16);
    for (int t = 0; t < n; ++t) { mask_at[(size_t)t] = o; o += align_up((size_t)descs[t].m, 16); }
    const size_t out_end = o;
    if (int rc = ensure_stage(ctx, out_end, out_end)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    for (int t = 0; t < n; ++t) {
        const dsdtm_homography_desc& d = descs[t];
        HomographyDev r;
        memset(&r, 0, sizeof r);
        r.a = (const float*)(g + a_at[(size_t)t]); r.b = (const float*)(g + b_at[(size_t)t]);
        r.mask = g + mask_at[(size_t)t];
        r.out = (dsdtm_homography_result*)(g + out_begin) + t;
        const double thr = d.reproj_threshold > 0.0 ? d.reproj_threshold : DSDTM_HOMOGRAPHY_DEFAULT_THRESHOLD;
        const double confidence = d.confidence > 0.0 ? d.confidence : DSDTM_HOMOGRAPHY_DEFAULT_CONFIDENCE;
        const int hyp = d.max_hypotheses > 0 ? d.max_hypotheses : DSDTM_HOMOGRAPHY_DEFAULT_HYPOTHESES;
        r.thr2 = thr * thr;
        r.left = 1.0 - confidence;
        r.m = d.m;
        r.rounds_max = (hyp + HOMOGRAPHY_ROUND - 1) / HOMOGRAPHY_ROUND;
        r.seed = d.seed ? d.seed : DSDTM_HOMOGRAPHY_DEFAULT_SEED;
        memcpy(h + (size_t)t * sizeof r, &r, sizeof r);
        if (d.m > 0) {
            memcpy(h + a_at[(size_t)t], d.points_a, (size_t)d.m * 8);
            memcpy(h + b_at[(size_t)t], d.points_b, (size_t)d.m * 8);
        }
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(homography_launch((const HomographyDev*)g, n, ctx->stream));
    API_TRY(hipMemcpyAsync(h + out_begin, g + out_begin, out_end - out_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        dsdtm_homography_result got;
        memcpy(&got, h + out_begin + (size_t)t * sizeof got, sizeof got);
        if (got.found != 1) { results[t].found = 0; continue; }          // nothing else is written
        results[t] = got;
        if (descs[t].mask) memcpy(descs[t].mask, h + mask_at[(size_t)t], (size_t)descs[t].m);
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_find_homography(dsdtm_homography_ctx* ctx, int m, const float* points_a, const float* points_b, uint8_t* mask,
                                     dsdtm_homography_result* result) {
    dsdtm_homography_desc d;
    memset(&d, 0, sizeof d);
    d.points_a = points_a; d.points_b = points_b; d.mask = mask; d.m = m;
    return dsdtm_find_homographies(ctx, 1, &d, result);
}
