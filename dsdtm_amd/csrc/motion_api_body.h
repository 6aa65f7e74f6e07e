// motion_api_body.h — the C ABI of include/dsdtm_amd_motion.h: contexts, models, checks, packing, launch (the context: addon_host.h).
// ONE implementation, compiled once per library that serves the models: the including translation unit names the entries
// (MO_API(steps) -> dsdtm_motion_steps in motion_api.cpp, dsdtm_mcd_model_create in mcd_api.cpp), the context and model types (MO_CTX,
// MO_MODEL) and the library as its messages call it (MO_LIB) before it includes this file. With MO_CONTOUR defined (mcd_api.cpp) run_steps
// also knows the contour step of contour.h; without it nothing of that is compiled and libdsdtm_amd_motion.so is what it was.
//
// A step packs the n models' records, host images and feature coordinates into one pinned block, moves it with a single
// hipMemcpyAsync, launches motion.hip's step kernel (and, where features were given, the lookup behind it) on the context's stream
// and reads the flags and the wanted masks back with one copy each into the pinned block; the caller's arrays are written only after
// the wait succeeded, and only then do the models turn to the generation the kernel wrote. There is no CPU compute path here.
#if !defined(MO_API) || !defined(MO_CTX) || !defined(MO_MODEL) || !defined(MO_LIB)
#error "motion_api_body.h: define MO_API(name), MO_CTX, MO_MODEL and MO_LIB before including it (see motion_api.cpp)"
#endif
#ifdef DSDTM_MOTION_API_BODY_H
#error "motion_api_body.h defines the entries of ONE library: include it once per translation unit"
#endif
#define DSDTM_MOTION_API_BODY_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "motion.h"
#ifdef MO_CONTOUR
#include "contour.h"
#endif
#include "addon_host.h"

using namespace dsdtm;

// (staging: the pinned block holds what is copied either way; the device block, at the same offsets, also the masks nobody asked
// for: the feature lookup reads them)
struct MO_CTX : dsdtm::AddonCtx {};

struct MO_MODEL {
    MO_CTX* ctx = nullptr;
    int width = 0, height = 0, mw = 0, mh = 0;
    size_t cells = 0;
    float* d_state = nullptr;      // 2 generations x 12 arrays x cells
    int gen = 0;                   // the generation that holds the model
    float* generation(int g) const { return d_state + (size_t)g * MOTION_ARRAYS * cells; }
};

extern "C" const char* MO_API(last_error)(const MO_CTX* ctx) { return addon_last_error(ctx); }
extern "C" int MO_API(create)(int device, MO_CTX** out) { return addon_create(MO_LIB, device, out); }
extern "C" void MO_API(destroy)(MO_CTX* ctx) { addon_destroy(ctx); }

// Where an image of the caller lives (0: host memory, ordinary or pinned; 2: this device's memory; -1: another device's)
static int image_memory(MO_CTX* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return 0; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? 2 : -1;
    return 0;
}

// ProbModel::init on the device: one step from an all-zero model on an all-zero image with the identity, into the generation that
// does not hold the model (a reset that fails leaves it as it was)
static int model_init(MO_CTX* ctx, MO_MODEL* m) {
    if (int rc = ensure_stage(ctx, sizeof(MotionStepDev), sizeof(MotionStepDev))) return rc;
    MotionStepDev r;
    memset(&r, 0, sizeof r);
    r.src = nullptr; r.dst = m->generation(1 - m->gen);
    r.H[0] = r.H[4] = r.H[8] = 1.0;
    r.width = m->width; r.height = m->height; r.mw = m->mw; r.mh = m->mh;
    memcpy(ctx->h_pinned, &r, sizeof r);
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage, ctx->h_pinned, sizeof r, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(motion_step_launch((const MotionStepDev*)ctx->d_stage, 1, (m->mw + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS,
                               (m->mh + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    m->gen = 1 - m->gen;
    return DSDTM_OK;
}

extern "C" int MO_API(model_create)(MO_CTX* ctx, int width, int height, MO_MODEL** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "model_create: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    if (width < DSDTM_MOTION_MIN_SIDE || width > DSDTM_MOTION_MAX_SIDE) { set_err(ctx, "model_create: width = %d outside %d..%d", width, DSDTM_MOTION_MIN_SIDE, DSDTM_MOTION_MAX_SIDE); return DSDTM_ERR_INVALID; }
    if (height < DSDTM_MOTION_MIN_SIDE || height > DSDTM_MOTION_MAX_SIDE) { set_err(ctx, "model_create: height = %d outside %d..%d", height, DSDTM_MOTION_MIN_SIDE, DSDTM_MOTION_MAX_SIDE); return DSDTM_ERR_INVALID; }
    MO_MODEL* m = new (std::nothrow) MO_MODEL();
    if (!m) return DSDTM_ERR_NOMEM;
    m->ctx = ctx; m->width = width; m->height = height; m->mw = width / 4; m->mh = height / 4;
    m->cells = (size_t)m->mw * (size_t)m->mh;
    int rc = DSDTM_OK;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void**)&m->d_state, sizeof(float) * 2 * MOTION_ARRAYS * m->cells) != hipSuccess) {
        set_err(ctx, "model_create: hipMalloc of %zu bytes failed", sizeof(float) * 2 * MOTION_ARRAYS * m->cells);
        m->d_state = nullptr;
        rc = DSDTM_ERR_HIP;
    } else rc = model_init(ctx, m);
    if (rc != DSDTM_OK) {
        if (m->d_state) (void)hipFree(m->d_state);
        delete m;
        return rc;
    }
    *out = m;
    return DSDTM_OK;
}

extern "C" void MO_API(model_destroy)(MO_CTX* ctx, MO_MODEL* model) {
    if (!model) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    if (model->d_state) (void)hipFree(model->d_state);
    delete model;
}

static int check_model(MO_CTX* ctx, const MO_MODEL* model, const char* who) {
    if (!model) { set_err(ctx, "%s: model is NULL", who); return DSDTM_ERR_INVALID; }
    if (model->ctx != ctx) { set_err(ctx, "%s: model belongs to another context", who); return DSDTM_ERR_INVALID; }
    return DSDTM_OK;
}

extern "C" int MO_API(model_reset)(MO_CTX* ctx, MO_MODEL* model) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (int rc = check_model(ctx, model, "model_reset")) return rc;
    return model_init(ctx, model);
}

extern "C" int MO_API(model_read)(MO_CTX* ctx, const MO_MODEL* model, float* out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (int rc = check_model(ctx, model, "model_read")) return rc;
    if (!out) { set_err(ctx, "model_read: out is NULL"); return DSDTM_ERR_INVALID; }
    const size_t bytes = sizeof(float) * MOTION_ARRAYS * model->cells;
    if (int rc = ensure_stage(ctx, bytes, 0)) return rc;
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, model->generation(model->gen), bytes, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->h_pinned, bytes);
    return DSDTM_OK;
}

extern "C" int MO_API(model_write)(MO_CTX* ctx, MO_MODEL* model, const float* in) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (int rc = check_model(ctx, model, "model_write")) return rc;
    if (!in) { set_err(ctx, "model_write: in is NULL"); return DSDTM_ERR_INVALID; }
    const size_t bytes = sizeof(float) * MOTION_ARRAYS * model->cells;
    if (int rc = ensure_stage(ctx, bytes, 0)) return rc;
    memcpy(ctx->h_pinned, in, bytes);
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    // into the generation that does not hold the model: a copy that fails leaves it as it was
    HIP_TRY(ctx, hipMemcpyAsync(model->generation(1 - model->gen), ctx->h_pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    model->gen = 1 - model->gen;
    return DSDTM_OK;
}

// cvRound of a float under the default rounding mode: to nearest, halves to even
static float cv_round(float v) { return nearbyintf(v); }

// One model's step as the entries of either library hand it to run_steps. `mask` is detect_img as update() leaves it; the fields behind
// `contour` are read only with MO_CONTOUR (the whole MCDWrapper::Run: `boxed` receives the image with the rectangle, `result` C3-C5).
struct StepArgs {
    MO_MODEL* model;
    const uint8_t* image; int32_t stride;
    int32_t mask_stride; uint8_t* mask;
    const double* H;
    int32_t n_features;
    const float* feature_px; uint8_t* feature_on_mask;
    int32_t boxed_stride; uint8_t* boxed;
};

// what is wrong with one step, or nullptr; `detail` receives the feature index where one is named
static const char* check_step(MO_CTX* ctx, const StepArgs& d, bool contour, int* mem, int* detail) {
    *detail = -1;
    if (!d.model) return "model is NULL";
    if (d.model->ctx != ctx) return "model belongs to another context";
    const int w = d.model->width, h = d.model->height;
    if (!d.image) return "image is NULL";
    if (d.stride < w) return "stride is smaller than the width";
    if (!d.H) return "H is NULL";
    for (int k = 0; k < 9; ++k) if (!std::isfinite(d.H[k])) return "H is not finite";
    for (int corner = 0; corner < 4; ++corner) {          // :185-189 at the four corner cells
        const float X = (float)(4.0 * ((corner & 1) ? d.model->mw - 1 : 0) + 4.0 / 2.0), Y = (float)(4.0 * ((corner & 2) ? d.model->mh - 1 : 0) + 4.0 / 2.0);
        const float newW = (float)(d.H[6] * X + d.H[7] * Y + d.H[8]);
        if (!(newW > 0) || !std::isfinite(newW)) return "H: the denominator h6 * X + h7 * Y + h8 is not positive at a corner cell";
    }
    if (d.mask && d.mask_stride < w) return contour ? "mask_raw_stride is smaller than the width" : "mask_stride is smaller than the width";
    if (contour && d.boxed && d.boxed_stride < w) return "mask_stride is smaller than the width";
    if (d.n_features < 0 || d.n_features > DSDTM_MOTION_MAX_FEATURES) return "n_features out of range";
    if (d.n_features > 0 && !d.feature_px) return "feature_px is NULL";
    if (d.n_features > 0 && !d.feature_on_mask) return "feature_on_mask is NULL";
    for (int f = 0; f < d.n_features; ++f) {
        const float x = d.feature_px[2 * (size_t)f], y = d.feature_px[2 * (size_t)f + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) { *detail = f; return "feature_px is not finite at feature"; }
        const float rx = cv_round(x), ry = cv_round(y);
        if (rx < 0 || rx >= (float)w || ry < 0 || ry >= (float)h) { *detail = f; return "feature_px rounds outside the image at feature"; }
    }
    *mem = image_memory(ctx, d.image);
    if (*mem < 0) return "image lies in another device's memory";
    return nullptr;
}

#ifdef MO_CONTOUR
// The masks of recs[0 .. n) go through contour.hip in runs whose scratch fits `scratch_bytes` at `scratch` (a run's launches follow the
// previous run's on the stream, so the runs share it): binds every record's scratch on the way. At least one mask per run.
struct ContourRun { int first, count, max_pixels; };
static std::vector<ContourRun> contour_runs(std::vector<ContourDev>& recs, uint8_t* scratch, size_t scratch_bytes) {
    std::vector<ContourRun> runs;
    size_t used = 0;
    for (int t = 0; t < (int)recs.size(); ++t) {
        const size_t need = contour_scratch_bytes(recs[(size_t)t].width, recs[(size_t)t].height);
        if (runs.empty() || used + need > scratch_bytes) { runs.push_back(ContourRun{t, 0, 0}); used = 0; }
        contour_bind_scratch(recs[(size_t)t], scratch + used);
        used += need;
        runs.back().count += 1;
        runs.back().max_pixels = std::max(runs.back().max_pixels, recs[(size_t)t].width * recs[(size_t)t].height);
    }
    return runs;
}
// what the runs need at most: the budget, or the one mask that is larger than it
static size_t contour_scratch_need(const std::vector<ContourDev>& recs) {
    size_t total = 0, largest = 0;
    for (const ContourDev& r : recs) { const size_t b = contour_scratch_bytes(r.width, r.height); total += b; largest = std::max(largest, b); }
    return std::max(largest, std::min(total, (size_t)CONTOUR_SCRATCH_BUDGET));
}
#endif

// `results`: with MO_CONTOUR and contour, n records that receive C3-C5 after the wait; `who` names the entry in messages
static int run_steps(MO_CTX* ctx, const char* who, int n, const StepArgs* descs, bool contour, void* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MOTION_STEPS_MAX) { set_err(ctx, "%s: n = %d outside 0..%d", who, n, DSDTM_MOTION_STEPS_MAX); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "%s: descs is NULL", who); return DSDTM_ERR_INVALID; }
#ifndef MO_CONTOUR
    (void)results;
    contour = false;
#endif
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   records | contour records | host images (pitch = width up to 16) | feature coordinates || flags | contour results |
    //   masks (pitch = width up to 16) || pinned only: the masks before the rectangle; device only: the contour step's scratch
    const size_t N = (size_t)n;
    std::vector<MotionStepDev> rec(N);
    std::vector<size_t> img_at(N, 0), feat_at(N, 0), flag_at(N, 0), mask_at(N, 0);
    std::vector<int> mem(N, 0);
    size_t o = align_up(N * sizeof(MotionStepDev), 256);
#ifdef MO_CONTOUR
    const size_t crec_at = o;
    std::vector<ContourDev> crec(contour ? N : 0);
    if (contour) o = align_up(o + N * sizeof(ContourDev), 256);
#endif
    int tiles_x = 0, tiles_y = 0, max_feat = 0;
    for (int t = 0; t < n; ++t) {
        const StepArgs& d = descs[t];
        int detail = -1;
        if (const char* bad = check_step(ctx, d, contour, &mem[(size_t)t], &detail)) {
            if (detail >= 0) set_err(ctx, "%s: model %d: %s %d", who, t, bad, detail);
            else set_err(ctx, "%s: model %d: %s", who, t, bad);
            return DSDTM_ERR_INVALID;
        }
        const MO_MODEL* m = d.model;
#ifdef MO_CONTOUR
        if (contour && (int64_t)m->width * m->height > CONTOUR_MAX_PIXELS) {
            set_err(ctx, "%s: model %d: %d x %d = %lld pixels, the contour step takes %d at most", who, t, m->width, m->height, (long long)m->width * m->height, CONTOUR_MAX_PIXELS);
            return DSDTM_ERR_INVALID;
        }
#endif
        if (mem[(size_t)t] == 0) { img_at[(size_t)t] = o; o += align_up((size_t)m->width, 16) * (size_t)m->height; }
        if (d.n_features > 0) { feat_at[(size_t)t] = o; o += align_up((size_t)d.n_features * 8, 16); }
        tiles_x = std::max(tiles_x, (m->mw + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS);
        tiles_y = std::max(tiles_y, (m->mh + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS);
        max_feat = std::max(max_feat, (int)d.n_features);
    }
    {   // the same model twice would be written by two grid slices at once
        std::vector<const MO_MODEL*> seen(N);
        for (int t = 0; t < n; ++t) seen[(size_t)t] = descs[t].model;
        std::sort(seen.begin(), seen.end());
        for (size_t k = 1; k < N; ++k)
            if (seen[k] == seen[k - 1]) {
                int first = -1, second = -1;
                for (int t = 0; t < n; ++t) if (descs[t].model == seen[k]) { if (first < 0) first = t; else if (second < 0) second = t; }
                set_err(ctx, "%s: model %d: model is the same as that of model %d", who, second, first);
                return DSDTM_ERR_INVALID;
            }
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t flags_begin = o;
    for (int t = 0; t < n; ++t) if (descs[t].n_features > 0) { flag_at[(size_t)t] = o; o += align_up((size_t)descs[t].n_features, 16); }
#ifdef MO_CONTOUR
    const size_t result_at = align_up(o, 16);
    if (contour) o = result_at + N * sizeof(ContourResult);
#endif
    const size_t flags_end = o;                     // (with the contour step: the flags and the results, one copy)
    o = align_up(o, 256);
    size_t copy_begin = 0, copy_end = 0;            // the span of the masks somebody wants: detect_img ...
    size_t boxed_begin = 0, boxed_end = 0;          // ... and with the rectangle
    for (int t = 0; t < n; ++t) {
        const StepArgs& d = descs[t];
        if (!contour && !d.mask && d.n_features == 0) continue;
        mask_at[(size_t)t] = o;
        o += align_up((size_t)d.model->width, MOTION_MASK_ALIGN) * (size_t)d.model->height;
        if (d.mask) { if (!copy_end) copy_begin = mask_at[(size_t)t]; copy_end = o; }
        if (contour && d.boxed) { if (!boxed_end) boxed_begin = mask_at[(size_t)t]; boxed_end = o; }
    }
    size_t d_bytes = o, h_bytes = std::max(copy_end, boxed_end) ? std::max(copy_end, boxed_end) : flags_end;
    // detect_img leaves the device before the rectangle is drawn into it, into an area of its own behind the block
    const size_t raw_at = align_up(h_bytes, 256);
    if (contour && copy_end) h_bytes = raw_at + (copy_end - copy_begin);
#ifdef MO_CONTOUR
    const size_t scratch_at = align_up(d_bytes, 256);
    size_t scratch_bytes = 0;
    if (contour) {
        for (int t = 0; t < n; ++t) { crec[(size_t)t].width = descs[t].model->width; crec[(size_t)t].height = descs[t].model->height; }
        scratch_bytes = contour_scratch_need(crec);
        d_bytes = scratch_at + scratch_bytes;
    }
#endif
    if (int rc = ensure_stage(ctx, h_bytes, d_bytes)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    for (int t = 0; t < n; ++t) {
        const StepArgs& d = descs[t];
        const MO_MODEL* m = d.model;
        MotionStepDev& r = rec[(size_t)t];
        memset(&r, 0, sizeof r);
        const size_t pitch = align_up((size_t)m->width, 16);
        if (mem[(size_t)t] == 0) {
            for (int y = 0; y < m->height; ++y) memcpy(h + img_at[(size_t)t] + (size_t)y * pitch, d.image + (size_t)y * (size_t)d.stride, (size_t)m->width);
            r.image = g + img_at[(size_t)t]; r.img_stride = (int32_t)pitch;
        } else { r.image = d.image; r.img_stride = d.stride; }
        r.src = m->generation(m->gen); r.dst = m->generation(1 - m->gen);
        if (mask_at[(size_t)t]) { r.mask = g + mask_at[(size_t)t]; r.mask_pitch = (int32_t)align_up((size_t)m->width, MOTION_MASK_ALIGN); }
        if (d.n_features > 0) {
            memcpy(h + feat_at[(size_t)t], d.feature_px, (size_t)d.n_features * 8);
            r.feat = (const float*)(g + feat_at[(size_t)t]); r.flags = g + flag_at[(size_t)t];
        }
        r.n_feat = d.n_features;
        memcpy(r.H, d.H, sizeof r.H);
        r.width = m->width; r.height = m->height; r.mw = m->mw; r.mh = m->mh;
    }
    memcpy(h, rec.data(), N * sizeof(MotionStepDev));
#ifdef MO_CONTOUR
    std::vector<ContourRun> runs;
    if (contour) {
        for (int t = 0; t < n; ++t) {           // the rectangle is drawn into detect_img where it lies: the lookup behind it reads it there
            ContourDev& c = crec[(size_t)t];
            c.src = rec[(size_t)t].mask; c.dst = rec[(size_t)t].mask; c.src_pitch = c.dst_pitch = rec[(size_t)t].mask_pitch;
            c.result = (ContourResult*)(g + result_at) + t;
        }
        runs = contour_runs(crec, g + scratch_at, scratch_bytes);
        memcpy(h + crec_at, crec.data(), N * sizeof(ContourDev));
    }
#endif
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(motion_step_launch((const MotionStepDev*)g, n, tiles_x, tiles_y, ctx->stream));
#ifdef MO_CONTOUR
    if (contour) {
        if (copy_end) API_TRY(hipMemcpyAsync(h + raw_at, g + copy_begin, copy_end - copy_begin, hipMemcpyDeviceToHost, ctx->stream));
        for (const ContourRun& run : runs) API_TRY(contour_launch((const ContourDev*)(g + crec_at) + run.first, run.count, run.max_pixels, ctx->stream));
        int max_pixels = 0;
        for (const ContourRun& run : runs) max_pixels = std::max(max_pixels, run.max_pixels);
        API_TRY(contour_fill_launch((const ContourDev*)(g + crec_at), n, max_pixels, ctx->stream));
    }
#endif
    if (max_feat > 0) API_TRY(motion_features_launch((const MotionStepDev*)g, n, max_feat, ctx->stream));
    if (flags_end > flags_begin) API_TRY(hipMemcpyAsync(h + flags_begin, g + flags_begin, flags_end - flags_begin, hipMemcpyDeviceToHost, ctx->stream));
    if (!contour && copy_end) API_TRY(hipMemcpyAsync(h + copy_begin, g + copy_begin, copy_end - copy_begin, hipMemcpyDeviceToHost, ctx->stream));
    if (contour && boxed_end) API_TRY(hipMemcpyAsync(h + boxed_begin, g + boxed_begin, boxed_end - boxed_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
#ifdef MO_CONTOUR
    if (contour) {
        const ContourResult* got = (const ContourResult*)(h + result_at);
        for (int t = 0; t < n; ++t)
            if (got[t].status != 0) { set_err(ctx, "%s: model %d: a contour walk passed its cap of 4 * pixels + 4 steps", who, t); return DSDTM_ERR_HIP; }
        memcpy(results, got, N * sizeof(ContourResult));
    }
#endif
    for (int t = 0; t < n; ++t) {
        const StepArgs& d = descs[t];
        MO_MODEL* m = d.model;
        const size_t pitch = align_up((size_t)m->width, MOTION_MASK_ALIGN);
        if (d.n_features > 0) memcpy(d.feature_on_mask, h + flag_at[(size_t)t], (size_t)d.n_features);
        if (d.mask) {
            const uint8_t* from = contour ? h + raw_at + (mask_at[(size_t)t] - copy_begin) : h + mask_at[(size_t)t];
            for (int y = 0; y < m->height; ++y) memcpy(d.mask + (size_t)y * (size_t)d.mask_stride, from + (size_t)y * pitch, (size_t)m->width);
        }
        if (contour && d.boxed)
            for (int y = 0; y < m->height; ++y) memcpy(d.boxed + (size_t)y * (size_t)d.boxed_stride, h + mask_at[(size_t)t] + (size_t)y * pitch, (size_t)m->width);
        m->gen = 1 - m->gen;
    }
    return DSDTM_OK;
}
