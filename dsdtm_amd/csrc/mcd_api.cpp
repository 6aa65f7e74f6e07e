// mcd_api.cpp — the C ABI of include/dsdtm_amd_mcd.h (libdsdtm_amd_mcd.so). Contexts, models and the step are the ONE implementation of
// motion_api_body.h, compiled here under the dsdtm_mcd_* names with the contour step switched on (MO_CONTOUR: behind the step kernel the
// launches of contour.hip, the rectangle drawn into detect_img where it lies, the feature lookup on that); behind them dsdtm_mcd_boxes,
// the same launches on masks of the caller: one upload, the contour launches, the fill, one read-back, one wait. There is no CPU
// compute path here (the host evaluation is host/dsdtm_mcd_host.hpp, which needs no library).
#include "../../include/dsdtm_amd_mcd.h"
#define MO_API(name) dsdtm_mcd_##name
#define MO_CTX dsdtm_mcd_ctx
#define MO_MODEL dsdtm_mcd_model
#define MO_LIB "dsdtm_amd_mcd"
#define MO_CONTOUR 1
#include "motion_api_body.h"

extern "C" int dsdtm_mcd_steps(dsdtm_mcd_ctx* ctx, int n, dsdtm_mcd_desc* descs) {
    std::vector<StepArgs> a;
    std::vector<ContourResult> res;
    if (ctx && descs && n > 0 && n <= DSDTM_MOTION_STEPS_MAX) {
        a.resize((size_t)n);
        res.resize((size_t)n);
        for (int t = 0; t < n; ++t) {
            const dsdtm_mcd_desc& d = descs[t];
            a[(size_t)t] = StepArgs{d.model, d.image, d.stride, d.mask_raw_stride, d.mask_raw, d.H, d.n_features, d.feature_px, d.feature_on_mask, d.mask_stride, d.mask};
        }
    }
    const int rc = run_steps(ctx, "mcd_steps", n, a.empty() ? nullptr : a.data(), true, res.data());
    if (rc != DSDTM_OK) return rc;
    for (int t = 0; t < n; ++t) {
        memcpy(descs[t].box, res[(size_t)t].box, sizeof descs[t].box);
        descs[t].area2 = res[(size_t)t].area2; descs[t].n_components = res[(size_t)t].n_components;
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_mcd_step(dsdtm_mcd_ctx* ctx, dsdtm_mcd_model* model, const uint8_t* image, int stride, const double* H,
                              uint8_t* mask_raw, int mask_raw_stride, uint8_t* mask, int mask_stride,
                              int n_features, const float* feature_px, uint8_t* feature_on_mask, int32_t* box, int64_t* area2, int32_t* n_components) {
    dsdtm_mcd_desc d;
    memset(&d, 0, sizeof d);
    d.model = model; d.image = image; d.stride = stride; d.H = H; d.mask_raw = mask_raw; d.mask_raw_stride = mask_raw_stride;
    d.mask = mask; d.mask_stride = mask_stride; d.n_features = n_features; d.feature_px = feature_px; d.feature_on_mask = feature_on_mask;
    const int rc = dsdtm_mcd_steps(ctx, 1, &d);
    if (rc != DSDTM_OK) return rc;
    if (box) memcpy(box, d.box, sizeof d.box);
    if (area2) *area2 = d.area2;
    if (n_components) *n_components = d.n_components;
    return DSDTM_OK;
}

extern "C" int dsdtm_mcd_boxes(dsdtm_mcd_ctx* ctx, int n, dsdtm_mcd_box_desc* descs) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MOTION_STEPS_MAX) { set_err(ctx, "mcd_boxes: n = %d outside 0..%d", n, DSDTM_MOTION_STEPS_MAX); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "mcd_boxes: descs is NULL"); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   contour records | host masks (pitch = width up to 16) || results | masks with the rectangle (pitch = width up to 16) || scratch
    const size_t N = (size_t)n;
    std::vector<ContourDev> crec(N);
    std::vector<size_t> src_at(N, 0), dst_at(N, 0);
    std::vector<int> mem(N, 0);
    size_t o = align_up(N * sizeof(ContourDev), 256);
    for (int t = 0; t < n; ++t) {
        const dsdtm_mcd_box_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.mask) bad = "mask is NULL";
        else if (d.width < DSDTM_MOTION_MIN_SIDE || d.width > DSDTM_MOTION_MAX_SIDE) bad = "width out of range";
        else if (d.height < DSDTM_MOTION_MIN_SIDE || d.height > DSDTM_MOTION_MAX_SIDE) bad = "height out of range";
        else if (d.stride < d.width) bad = "stride is smaller than the width";
        else if (d.boxed && d.boxed_stride < d.width) bad = "boxed_stride is smaller than the width";
        if (bad) { set_err(ctx, "mcd_boxes: mask %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        if ((int64_t)d.width * d.height > CONTOUR_MAX_PIXELS) {
            set_err(ctx, "mcd_boxes: mask %d: %d x %d = %lld pixels, the contour step takes %d at most", t, d.width, d.height, (long long)d.width * d.height, CONTOUR_MAX_PIXELS);
            return DSDTM_ERR_INVALID;
        }
        mem[(size_t)t] = image_memory(ctx, d.mask);
        if (mem[(size_t)t] < 0) { set_err(ctx, "mcd_boxes: mask %d: mask lies in another device's memory", t); return DSDTM_ERR_INVALID; }
        if (mem[(size_t)t] == 0) { src_at[(size_t)t] = o; o += align_up((size_t)d.width, 16) * (size_t)d.height; }
        crec[(size_t)t].width = d.width; crec[(size_t)t].height = d.height;
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t back_begin = o;
    o += N * sizeof(ContourResult);
    size_t back_end = o;
    o = align_up(o, 256);
    for (int t = 0; t < n; ++t)
        if (descs[t].boxed) { dst_at[(size_t)t] = o; o += align_up((size_t)descs[t].width, 16) * (size_t)descs[t].height; back_end = o; }
    const size_t scratch_at = align_up(o, 256), scratch_bytes = contour_scratch_need(crec);
    if (int rc = ensure_stage(ctx, back_end, scratch_at + scratch_bytes)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    int max_pixels = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_mcd_box_desc& d = descs[t];
        ContourDev& c = crec[(size_t)t];
        const size_t pitch = align_up((size_t)d.width, 16);
        if (mem[(size_t)t] == 0) {
            for (int y = 0; y < d.height; ++y) memcpy(h + src_at[(size_t)t] + (size_t)y * pitch, d.mask + (size_t)y * (size_t)d.stride, (size_t)d.width);
            c.src = g + src_at[(size_t)t]; c.src_pitch = (int32_t)pitch;
        } else { c.src = d.mask; c.src_pitch = d.stride; }
        if (d.boxed) { c.dst = g + dst_at[(size_t)t]; c.dst_pitch = (int32_t)pitch; }
        c.result = (ContourResult*)(g + back_begin) + t;
        max_pixels = std::max(max_pixels, d.width * d.height);
    }
    const std::vector<ContourRun> runs = contour_runs(crec, g + scratch_at, scratch_bytes);
    memcpy(h, crec.data(), N * sizeof(ContourDev));
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    for (const ContourRun& run : runs) API_TRY(contour_launch((const ContourDev*)g + run.first, run.count, run.max_pixels, ctx->stream));
    if (back_end > back_begin + N * sizeof(ContourResult)) API_TRY(contour_fill_launch((const ContourDev*)g, n, max_pixels, ctx->stream));
    API_TRY(hipMemcpyAsync(h + back_begin, g + back_begin, back_end - back_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    const ContourResult* got = (const ContourResult*)(h + back_begin);
    for (int t = 0; t < n; ++t)
        if (got[t].status != 0) { set_err(ctx, "mcd_boxes: mask %d: a contour walk passed its cap of 4 * pixels + 4 steps", t); return DSDTM_ERR_HIP; }
    for (int t = 0; t < n; ++t) {
        dsdtm_mcd_box_desc& d = descs[t];
        memcpy(d.box, got[t].box, sizeof d.box);
        d.area2 = got[t].area2; d.n_components = got[t].n_components;
        if (d.boxed) {
            const size_t pitch = align_up((size_t)d.width, 16);
            for (int y = 0; y < d.height; ++y) memcpy(d.boxed + (size_t)y * (size_t)d.boxed_stride, h + dst_at[(size_t)t] + (size_t)y * pitch, (size_t)d.width);
        }
    }
    return DSDTM_OK;
}
