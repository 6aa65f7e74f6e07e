// framediff_api.cpp — the C ABI of include/dsdtm_amd_framediff.h (libdsdtm_amd_framediff.so): checks, F1, staging, launches (the
// context: addon_host.h).
//
// dsdtm_framediff_steps checks every desc and inverts every H (F1, host/dsdtm_framediff_host.hpp's function: ONE definition for the
// library and the host path), lays ONE block out
//     records | every pageable source, packed | feature coordinates | counters || flags | every host output, packed | (device only: the
//     masks nobody asked for but a feature test reads)
// fills the pinned side, moves the front (counters included: they start at zero) with a single hipMemcpyAsync, launches framediff.hip's
// kernel once for all pairs and the feature test behind it, copies counters, flags and host outputs back with one copy and waits once;
// the caller's memory is written only after the wait succeeded. There is no CPU compute path here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "framediff.h"
#include "addon_host.h"
#include "../host/dsdtm_framediff_host.hpp"

using namespace dsdtm;

struct dsdtm_framediff_ctx : dsdtm::AddonCtx {};

extern "C" const char* dsdtm_framediff_last_error(const dsdtm_framediff_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_framediff_create(int device, dsdtm_framediff_ctx** out) { return addon_create("dsdtm_amd_framediff", device, out); }
extern "C" void dsdtm_framediff_destroy(dsdtm_framediff_ctx* ctx) { addon_destroy(ctx); }

static bool capturing(dsdtm_framediff_ctx* ctx) {      // (every entry allocates or waits: neither can be part of a capture)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return cs != hipStreamCaptureStatusNone;
}

// ---- where a caller's image lies: THE rule for the four images of a desc
enum { MEM_PAGEABLE = 0, MEM_PINNED = 1, MEM_DEVICE = 2, MEM_OTHER_DEVICE = -1 };
static int array_memory(const dsdtm_framediff_ctx* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return MEM_PAGEABLE; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? MEM_DEVICE : MEM_OTHER_DEVICE;
    if (pa_.type == hipMemoryTypeHost) return MEM_PINNED;
    return MEM_PAGEABLE;
}

enum { IMG_A = 0, IMG_B = 1, IMG_MASK = 2, IMG_WARPED = 3 };
static const char* const IMG_NAME[4] = {"a", "b", "mask", "warped"};
struct Image {
    const void* p = nullptr;
    size_t stride = 0;
    int mem = MEM_PAGEABLE;
    size_t off = 0;                   // where in the block: a pageable source, a host output (packed: stride = width)
};
struct PairPlan {
    Image img[4];
    double M[9];
    size_t feat_off = 0, flag_off = 0, scratch_off = 0;
    bool scratch_mask = false;        // no mask wanted, features given: the kernel writes one that stays on the device
};
struct Extent { uintptr_t lo, hi; int pair, what; };

static float cv_round(float v) { return std::nearbyintf(v); }      // halves to even: the default rounding mode

// what is wrong with one desc, or nullptr; `detail` receives the feature index where one is named
static const char* check_desc(const dsdtm_framediff_desc& d, bool warp_only, double M[9], int* detail) {
    *detail = -1;
    if (!warp_only && !d.a) return "a is NULL";
    if (!d.b) return "b is NULL";
    if (d.width < DSDTM_FRAMEDIFF_MIN_SIDE || d.width > DSDTM_FRAMEDIFF_MAX_SIDE) return "width out of range";
    if (d.height < DSDTM_FRAMEDIFF_MIN_SIDE || d.height > DSDTM_FRAMEDIFF_MAX_SIDE) return "height out of range";
    if (!warp_only && d.a_stride < d.width) return "a_stride below width";
    if (d.b_stride < d.width) return "b_stride below width";
    if (d.flags & ~DSDTM_FRAMEDIFF_INVERSE_MAP) return "flags has unknown bits";
    if (!warp_only && (d.threshold < 0 || d.threshold > 254)) return "threshold outside 0..254";
    if (!warp_only && (d.maxval < 0 || d.maxval > 255)) return "maxval outside 0..255";
    for (int k = 0; k < 9; ++k) if (!std::isfinite(d.H[k])) return "H is not finite";
    if (!DSDTM::framediff_matrix_host(d.H, d.flags, M)) return "H is singular or its inverse is not finite";
    if (warp_only && !d.warped) return "warped is NULL";
    if (d.warped && d.warped_stride < d.width) return "warped_stride below width";
    if (warp_only) return nullptr;
    if (d.mask && d.mask_stride < d.width) return "mask_stride below width";
    if (d.n_features < 0 || d.n_features > DSDTM_FRAMEDIFF_MAX_FEATURES) return "n_features out of range";
    if (d.n_features > 0 && !d.feature_px) return "feature_px is NULL";
    if (d.n_features > 0 && !d.feature_on_mask) return "feature_on_mask is NULL";
    for (int f = 0; f < d.n_features; ++f) {
        const float x = d.feature_px[2 * (size_t)f], y = d.feature_px[2 * (size_t)f + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) { *detail = f; return "feature_px is not finite at feature"; }
        const float rx = cv_round(x), ry = cv_round(y);
        if (rx < 0 || rx >= (float)d.width || ry < 0 || ry >= (float)d.height) { *detail = f; return "feature_px rounds outside the image at feature"; }
    }
    return nullptr;
}

// THE body of the three entries. warp_only: dsdtm_framediff_warp (results is NULL and a, mask, the features are not read).
static int run(dsdtm_framediff_ctx* ctx, const char* who, int n, const dsdtm_framediff_desc* descs, dsdtm_framediff_result* results, bool warp_only) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_FRAMEDIFF_MAX_STEPS) { set_err(ctx, "%s: n = %d outside 0..%d", who, n, DSDTM_FRAMEDIFF_MAX_STEPS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "%s: descs is NULL", who); return DSDTM_ERR_INVALID; }
    if (!warp_only && !results) { set_err(ctx, "%s: results is NULL", who); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "%s: not inside a stream capture", who); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    std::vector<PairPlan> plan(N);
    std::vector<Extent> extents;
    extents.reserve(4 * N);
    int max_w = 0, max_h = 0, max_feat = 0;
    size_t o = align_up(N * sizeof(FrameDiffDev), 256);
    for (int t = 0; t < n; ++t) {
        const dsdtm_framediff_desc& d = descs[t];
        PairPlan& p = plan[(size_t)t];
        int detail = -1;
        if (const char* bad = check_desc(d, warp_only, p.M, &detail)) {
            if (detail >= 0) set_err(ctx, "%s: desc %d: %s %d", who, t, bad, detail); else set_err(ctx, "%s: desc %d: %s", who, t, bad);
            return DSDTM_ERR_INVALID;
        }
        const size_t W = (size_t)d.width, H = (size_t)d.height;
        max_w = std::max(max_w, d.width); max_h = std::max(max_h, d.height);
        if (!warp_only) max_feat = std::max(max_feat, (int)d.n_features);
        const void* ptr[4] = {warp_only ? nullptr : d.a, d.b, warp_only ? nullptr : d.mask, d.warped};
        const int32_t stride[4] = {d.a_stride, d.b_stride, d.mask_stride, d.warped_stride};
        for (int k = 0; k < 4; ++k) {
            if (!ptr[k]) continue;
            Image& im = p.img[k];
            im.p = ptr[k]; im.stride = (size_t)stride[k];
            if (k == IMG_B && ptr[IMG_A] == ptr[IMG_B] && stride[IMG_A] == stride[IMG_B]) { im.mem = p.img[IMG_A].mem; im.off = p.img[IMG_A].off; continue; }      // QUIRK 1: staged once
            im.mem = array_memory(ctx, ptr[k]);
            if (im.mem == MEM_OTHER_DEVICE) { set_err(ctx, "%s: desc %d: %s lies in another device's memory", who, t, IMG_NAME[k]); return DSDTM_ERR_INVALID; }
            if (k <= IMG_B && im.mem == MEM_PAGEABLE) { im.off = o; o = align_up(o + W * H, 16); }
            const uintptr_t lo = (uintptr_t)ptr[k];
            extents.push_back(Extent{lo, lo + (H - 1) * im.stride + W, t, k});
        }
        if (!warp_only && d.n_features > 0) { p.feat_off = o; o = align_up(o + (size_t)d.n_features * 8, 16); }
    }
    const size_t counters = align_up(o, 256);
    const size_t upload = align_up(counters + N * sizeof(int32_t), 256);
    o = upload;
    for (int t = 0; t < n; ++t) {
        PairPlan& p = plan[(size_t)t];
        if (!warp_only && descs[t].n_features > 0) { p.flag_off = o; o = align_up(o + (size_t)descs[t].n_features, 16); }
        for (int k : {IMG_MASK, IMG_WARPED}) {
            Image& im = p.img[k];
            if (!im.p || im.mem == MEM_DEVICE) continue;
            im.off = o; o = align_up(o + (size_t)descs[t].width * (size_t)descs[t].height, 16);
        }
    }
    const size_t host_total = o;
    for (int t = 0; t < n; ++t) {
        PairPlan& p = plan[(size_t)t];
        if (warp_only || descs[t].mask || descs[t].n_features == 0) continue;
        p.scratch_mask = true; p.scratch_off = o; o = align_up(o + (size_t)descs[t].width * (size_t)descs[t].height, 16);
    }
    const size_t dev_total = o;
    {   // no output's extent meets an input's or another output's (a sweep over the extents in address order)
        std::sort(extents.begin(), extents.end(), [](const Extent& a, const Extent& b) { return a.lo < b.lo; });
        const Extent* far_dst = nullptr;      // the output / the image of any kind that reaches furthest so far
        const Extent* far_any = nullptr;
        for (const Extent& e : extents) {
            const bool is_dst = e.what >= IMG_MASK;
            const Extent* hit = is_dst ? far_any : far_dst;
            if (hit && e.lo < hit->hi) {
                const Extent& dst = is_dst ? e : *hit;
                const Extent& other = is_dst ? *hit : e;
                set_err(ctx, "%s: desc %d: %s overlaps %s of desc %d", who, dst.pair, IMG_NAME[dst.what], IMG_NAME[other.what], other.pair);
                return DSDTM_ERR_INVALID;
            }
            if (is_dst && (!far_dst || e.hi > far_dst->hi)) far_dst = &e;
            if (!far_any || e.hi > far_any->hi) far_any = &e;
        }
    }
    if (int rc = ensure_stage(ctx, host_total, dev_total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memset(h + counters, 0, N * sizeof(int32_t));
    for (int t = 0; t < n; ++t) {
        const dsdtm_framediff_desc& d = descs[t];
        const PairPlan& p = plan[(size_t)t];
        const size_t W = (size_t)d.width, H = (size_t)d.height;
        const void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t stride[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            const Image& im = p.img[k];
            if (!im.p) continue;
            stride[k] = im.stride;
            if (im.mem == MEM_DEVICE) dev[k] = im.p;
            else if (k >= IMG_MASK) { dev[k] = g + im.off; stride[k] = W; }                   // read back, packed
            else if (im.mem == MEM_PINNED) {
                void* v = nullptr;
                HIP_TRY(ctx, hipHostGetDevicePointer(&v, const_cast<void*>(im.p), 0));
                dev[k] = v;
            } else {                                                                          // pageable: packed into the upload
                if (!(k == IMG_B && p.img[IMG_A].p == im.p && p.img[IMG_A].off == im.off && p.img[IMG_A].mem == MEM_PAGEABLE))
                    for (size_t r = 0; r < H; ++r) memcpy(h + im.off + r * W, (const uint8_t*)im.p + r * im.stride, W);
                dev[k] = g + im.off; stride[k] = W;
            }
        }
        FrameDiffDev f;
        memset(&f, 0, sizeof f);
        memcpy(f.M, p.M, sizeof f.M);
        f.a = (const uint8_t*)dev[IMG_A]; f.b = (const uint8_t*)dev[IMG_B];
        f.mask = (uint8_t*)const_cast<void*>(dev[IMG_MASK]); f.warped = (uint8_t*)const_cast<void*>(dev[IMG_WARPED]);
        f.w = d.width; f.h = d.height;
        f.a_stride = (int32_t)stride[IMG_A]; f.b_stride = (int32_t)stride[IMG_B]; f.mask_stride = (int32_t)stride[IMG_MASK]; f.warped_stride = (int32_t)stride[IMG_WARPED];
        if (p.scratch_mask) { f.mask = g + p.scratch_off; f.mask_stride = d.width; }
        f.n_foreground = (int32_t*)(g + counters) + t;
        if (!warp_only) {
            f.threshold = d.threshold; f.maxval = d.maxval ? d.maxval : DSDTM_FRAMEDIFF_MAXVAL;
            f.n_feat = d.n_features;
            if (d.n_features > 0) {
                memcpy(h + p.feat_off, d.feature_px, (size_t)d.n_features * 8);
                f.feat = (const float*)(g + p.feat_off); f.flags = g + p.flag_off;
            }
        }
        memcpy(h + (size_t)t * sizeof f, &f, sizeof f);
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, upload, hipMemcpyHostToDevice, ctx->stream));
    if (warp_only) API_TRY(framediff_warp_launch((const FrameDiffDev*)g, n, max_w, max_h, ctx->stream));
    else {
        API_TRY(framediff_launch((const FrameDiffDev*)g, n, max_w, max_h, ctx->stream));
        if (max_feat > 0) API_TRY(framediff_features_launch((const FrameDiffDev*)g, n, max_feat, ctx->stream));
    }
    API_TRY(hipMemcpyAsync(h + counters, g + counters, host_total - counters, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const dsdtm_framediff_desc& d = descs[t];
        const PairPlan& p = plan[(size_t)t];
        for (int k : {IMG_MASK, IMG_WARPED}) {
            const Image& im = p.img[k];
            if (!im.p || im.mem == MEM_DEVICE) continue;
            const size_t row = (size_t)d.width;
            for (size_t r = 0; r < (size_t)d.height; ++r) memcpy((uint8_t*)const_cast<void*>(im.p) + r * im.stride, h + im.off + r * row, row);
        }
        if (warp_only) continue;
        dsdtm_framediff_result& res = results[t];
        memcpy(res.M, p.M, sizeof res.M);
        memcpy(&res.n_foreground, h + counters + (size_t)t * sizeof(int32_t), sizeof(int32_t));
        res.n_flagged = 0;
        if (d.n_features > 0) {
            memcpy(d.feature_on_mask, h + p.flag_off, (size_t)d.n_features);
            for (int f = 0; f < d.n_features; ++f) res.n_flagged += d.feature_on_mask[f];
        }
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_framediff_steps(dsdtm_framediff_ctx* ctx, int n, const dsdtm_framediff_desc* descs, dsdtm_framediff_result* results) {
    return run(ctx, "framediff_steps", n, descs, results, false);
}

extern "C" int dsdtm_framediff_step(dsdtm_framediff_ctx* ctx, const dsdtm_framediff_desc* desc, dsdtm_framediff_result* result) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!desc) { set_err(ctx, "framediff_step: desc is NULL"); return DSDTM_ERR_INVALID; }
    return run(ctx, "framediff_step", 1, desc, result, false);
}

extern "C" int dsdtm_framediff_warp(dsdtm_framediff_ctx* ctx, int n, const dsdtm_framediff_desc* descs) {
    return run(ctx, "framediff_warp", n, descs, nullptr, true);
}
