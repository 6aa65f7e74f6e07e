// motion_api.cpp — the C ABI of include/dsdtm_amd_motion.h (libdsdtm_amd_motion.so): models, checks, packing, launch (the context: addon_host.h).
//
// A step packs the n models' records, host images and feature coordinates into one pinned block, moves it with a single
// hipMemcpyAsync, launches motion.hip's step kernel (and, where features were given, the lookup behind it) on the context's stream
// and reads the flags and the wanted masks back with one copy each into the pinned block; the caller's arrays are written only after
// the wait succeeded, and only then do the models turn to the generation the kernel wrote. There is no CPU compute path here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "motion.h"
#include "addon_host.h"

using namespace dsdtm;

// (staging: the pinned block holds what is copied either way; the device block, at the same offsets, also the masks nobody asked
// for: the feature lookup reads them)
struct dsdtm_motion_ctx : dsdtm::AddonCtx {};

struct dsdtm_motion_model {
    dsdtm_motion_ctx* ctx = nullptr;
    int width = 0, height = 0, mw = 0, mh = 0;
    size_t cells = 0;
    float* d_state = nullptr;      // 2 generations x 12 arrays x cells
    int gen = 0;                   // the generation that holds the model
    float* generation(int g) const { return d_state + (size_t)g * MOTION_ARRAYS * cells; }
};

extern "C" const char* dsdtm_motion_last_error(const dsdtm_motion_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_motion_create(int device, dsdtm_motion_ctx** out) { return addon_create("dsdtm_amd_motion", device, out); }
extern "C" void dsdtm_motion_destroy(dsdtm_motion_ctx* ctx) { addon_destroy(ctx); }

// Where an image of the caller lives (0: host memory, ordinary or pinned; 2: this device's memory; -1: another device's)
static int image_memory(dsdtm_motion_ctx* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return 0; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? 2 : -1;
    return 0;
}

// ProbModel::init on the device: one step from an all-zero model on an all-zero image with the identity, into the generation that
// does not hold the model (a reset that fails leaves it as it was)
static int model_init(dsdtm_motion_ctx* ctx, dsdtm_motion_model* m) {
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

extern "C" int dsdtm_motion_model_create(dsdtm_motion_ctx* ctx, int width, int height, dsdtm_motion_model** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "model_create: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    if (width < DSDTM_MOTION_MIN_SIDE || width > DSDTM_MOTION_MAX_SIDE) { set_err(ctx, "model_create: width = %d outside %d..%d", width, DSDTM_MOTION_MIN_SIDE, DSDTM_MOTION_MAX_SIDE); return DSDTM_ERR_INVALID; }
    if (height < DSDTM_MOTION_MIN_SIDE || height > DSDTM_MOTION_MAX_SIDE) { set_err(ctx, "model_create: height = %d outside %d..%d", height, DSDTM_MOTION_MIN_SIDE, DSDTM_MOTION_MAX_SIDE); return DSDTM_ERR_INVALID; }
    dsdtm_motion_model* m = new (std::nothrow) dsdtm_motion_model();
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

extern "C" void dsdtm_motion_model_destroy(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model) {
    if (!model) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    if (model->d_state) (void)hipFree(model->d_state);
    delete model;
}

static int check_model(dsdtm_motion_ctx* ctx, const dsdtm_motion_model* model, const char* who) {
    if (!model) { set_err(ctx, "%s: model is NULL", who); return DSDTM_ERR_INVALID; }
    if (model->ctx != ctx) { set_err(ctx, "%s: model belongs to another context", who); return DSDTM_ERR_INVALID; }
    return DSDTM_OK;
}

extern "C" int dsdtm_motion_model_reset(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (int rc = check_model(ctx, model, "model_reset")) return rc;
    return model_init(ctx, model);
}

extern "C" int dsdtm_motion_model_read(dsdtm_motion_ctx* ctx, const dsdtm_motion_model* model, float* out) {
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

extern "C" int dsdtm_motion_model_write(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model, const float* in) {
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

// what is wrong with one desc, or nullptr; `detail` receives the feature index where one is named
static const char* check_desc(dsdtm_motion_ctx* ctx, const dsdtm_motion_desc& d, int* mem, int* detail) {
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
    if (d.mask && d.mask_stride < w) return "mask_stride is smaller than the width";
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

extern "C" int dsdtm_motion_steps(dsdtm_motion_ctx* ctx, int n, const dsdtm_motion_desc* descs) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MOTION_STEPS_MAX) { set_err(ctx, "motion_steps: n = %d outside 0..%d", n, DSDTM_MOTION_STEPS_MAX); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "motion_steps: descs is NULL"); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   records | host images (pitch = width up to 16) | feature coordinates || flags | masks (pitch = width up to 16)
    const size_t N = (size_t)n;
    std::vector<MotionStepDev> rec(N);
    std::vector<size_t> img_at(N, 0), feat_at(N, 0), flag_at(N, 0), mask_at(N, 0);
    std::vector<int> mem(N, 0);
    size_t o = align_up(N * sizeof(MotionStepDev), 256);
    int tiles_x = 0, tiles_y = 0, max_feat = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_motion_desc& d = descs[t];
        int detail = -1;
        if (const char* bad = check_desc(ctx, d, &mem[(size_t)t], &detail)) {
            if (detail >= 0) set_err(ctx, "motion_steps: model %d: %s %d", t, bad, detail);
            else set_err(ctx, "motion_steps: model %d: %s", t, bad);
            return DSDTM_ERR_INVALID;
        }
        const dsdtm_motion_model* m = d.model;
        if (mem[(size_t)t] == 0) { img_at[(size_t)t] = o; o += align_up((size_t)m->width, 16) * (size_t)m->height; }
        if (d.n_features > 0) { feat_at[(size_t)t] = o; o += align_up((size_t)d.n_features * 8, 16); }
        tiles_x = std::max(tiles_x, (m->mw + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS);
        tiles_y = std::max(tiles_y, (m->mh + MOTION_TILE_CELLS - 1) / MOTION_TILE_CELLS);
        max_feat = std::max(max_feat, (int)d.n_features);
    }
    {   // the same model twice would be written by two grid slices at once
        std::vector<const dsdtm_motion_model*> seen(N);
        for (int t = 0; t < n; ++t) seen[(size_t)t] = descs[t].model;
        std::sort(seen.begin(), seen.end());
        for (size_t k = 1; k < N; ++k)
            if (seen[k] == seen[k - 1]) {
                int first = -1, second = -1;
                for (int t = 0; t < n; ++t) if (descs[t].model == seen[k]) { if (first < 0) first = t; else if (second < 0) second = t; }
                set_err(ctx, "motion_steps: model %d: model is the same as that of model %d", second, first);
                return DSDTM_ERR_INVALID;
            }
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t flags_begin = o;
    for (int t = 0; t < n; ++t) if (descs[t].n_features > 0) { flag_at[(size_t)t] = o; o += align_up((size_t)descs[t].n_features, 16); }
    const size_t flags_end = o;
    o = align_up(o, 256);
    size_t copy_begin = 0, copy_end = 0;            // the span of the masks somebody wants
    for (int t = 0; t < n; ++t) {
        const dsdtm_motion_desc& d = descs[t];
        if (!d.mask && d.n_features == 0) continue;
        mask_at[(size_t)t] = o;
        o += align_up((size_t)d.model->width, MOTION_MASK_ALIGN) * (size_t)d.model->height;
        if (d.mask) { if (!copy_end) copy_begin = mask_at[(size_t)t]; copy_end = o; }
    }
    const size_t d_bytes = o, h_bytes = copy_end ? copy_end : flags_end;
    if (int rc = ensure_stage(ctx, h_bytes, d_bytes)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    for (int t = 0; t < n; ++t) {
        const dsdtm_motion_desc& d = descs[t];
        const dsdtm_motion_model* m = d.model;
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
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(motion_step_launch((const MotionStepDev*)g, n, tiles_x, tiles_y, ctx->stream));
    if (max_feat > 0) {
        API_TRY(motion_features_launch((const MotionStepDev*)g, n, max_feat, ctx->stream));
        API_TRY(hipMemcpyAsync(h + flags_begin, g + flags_begin, flags_end - flags_begin, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (copy_end) API_TRY(hipMemcpyAsync(h + copy_begin, g + copy_begin, copy_end - copy_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const dsdtm_motion_desc& d = descs[t];
        dsdtm_motion_model* m = d.model;
        if (d.n_features > 0) memcpy(d.feature_on_mask, h + flag_at[(size_t)t], (size_t)d.n_features);
        if (d.mask) {
            const size_t pitch = align_up((size_t)m->width, MOTION_MASK_ALIGN);
            for (int y = 0; y < m->height; ++y) memcpy(d.mask + (size_t)y * (size_t)d.mask_stride, h + mask_at[(size_t)t] + (size_t)y * pitch, (size_t)m->width);
        }
        m->gen = 1 - m->gen;
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_motion_step(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model, const uint8_t* image, int stride, const double* H,
                                 uint8_t* mask, int mask_stride, int n_features, const float* feature_px, uint8_t* feature_on_mask) {
    dsdtm_motion_desc d;
    memset(&d, 0, sizeof d);
    d.model = model; d.image = image; d.stride = stride; d.mask = mask; d.mask_stride = mask_stride; d.H = H;
    d.n_features = n_features; d.feature_px = feature_px; d.feature_on_mask = feature_on_mask;
    return dsdtm_motion_steps(ctx, 1, &d);
}
