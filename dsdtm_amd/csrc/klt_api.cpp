// klt_api.cpp — the C ABI of include/dsdtm_amd_klt.h (libdsdtm_amd_klt.so): checks, packing, launches (the context: addon_host.h).
//
// dsdtm_klt_steps packs the records, the grids and the host images of the n models into one pinned block and moves it with a single
// hipMemcpyAsync; then, on the context's stream: klt.hip's ingest launch (every level 0 into its model's spare pyramid), pyrdown.hip's
// launch per model and level, ONE Lucas-Kanade launch, the compaction launch (survivors and their count into the homography records
// on the device), homography.hip's launch, one copy back into the pinned block. The caller's arrays and the models are written only
// after the wait succeeded: then the pyramids are swapped. dsdtm_klt_flow is the same chain without models and without the homography,
// its pyramids in the device staging block. There is no CPU compute path here (that is host/dsdtm_klt_host.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "klt.h"
#include "kernels.h"
#include "addon_host.h"

using namespace dsdtm;

namespace {

// a packed pyramid: rows of level l are stride[l] apart (the width up to 16), levels start 256-byte aligned, 256 spare bytes behind the
// last (pyrdown.hip's wide loads may read, never use, a few bytes behind a row)
struct Geom {
    int levels = 0;
    int w[DSDTM_KLT_MAX_LEVELS] = {0}, h[DSDTM_KLT_MAX_LEVELS] = {0}, stride[DSDTM_KLT_MAX_LEVELS] = {0};
    uint32_t off[DSDTM_KLT_MAX_LEVELS] = {0};
    size_t bytes = 0;
};

Geom make_geom(int width, int height, int levels) {
    Geom g;
    g.levels = levels;
    size_t o = 0;
    for (int l = 0; l < levels; ++l) {
        g.w[l] = width; g.h[l] = height; g.stride[l] = (int)align_up((size_t)width, 16); g.off[l] = (uint32_t)o;
        o = align_up(o + (size_t)g.stride[l] * (size_t)height, 256);
        width = (width + 1) / 2; height = (height + 1) / 2;
    }
    g.bytes = o + 256;
    return g;
}

int grid_count(int width, int height, int gw, int gh) { return std::max(0, width / gw - 1) * std::max(0, height / gh - 1); }

void fill_dev(KltDev& r, const Geom& g) {
    for (int l = 0; l < g.levels; ++l) { r.w[l] = g.w[l]; r.h[l] = g.h[l]; r.stride[l] = g.stride[l]; r.off[l] = g.off[l]; }
    r.levels = g.levels;
}

}  // namespace

struct dsdtm_klt_ctx : dsdtm::AddonCtx {};

struct dsdtm_klt_model {
    int width = 0, height = 0;
    Geom geom;
    uint8_t* pyr[2] = {nullptr, nullptr};      // pyr[cur] holds the previous image's pyramid once frames > 0
    int cur = 0;
    int32_t frames = 0;
    double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
};

extern "C" const char* dsdtm_klt_last_error(const dsdtm_klt_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_klt_create(int device, dsdtm_klt_ctx** out) { return addon_create("dsdtm_amd_klt", device, out); }
extern "C" void dsdtm_klt_destroy(dsdtm_klt_ctx* ctx) { addon_destroy(ctx); }

static int image_memory(dsdtm_klt_ctx* ctx, const void* p) {      // 0: host memory, ordinary or pinned; 2: this device's; -1: another device's
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? 2 : -1;
    return 0;
}

static bool capturing(dsdtm_klt_ctx* ctx) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return cs != hipStreamCaptureStatusNone;
}

// what is wrong with a pyramid of `levels` levels for windows of `window`, or nullptr
static const char* check_pyramid(int width, int height, int levels, int window) {
    if (levels < 1 || levels > DSDTM_KLT_MAX_LEVELS) return "levels outside 1..5";
    if (window < DSDTM_KLT_MIN_WINDOW || window > DSDTM_KLT_MAX_WINDOW) return "window outside 3..21";
    if (width < 1 || width > 16384) return "width out of range";
    if (height < 1 || height > 16384) return "height out of range";
    for (int l = 1; l < levels; ++l) { width = (width + 1) / 2; height = (height + 1) / 2; }
    if (width < window + 3) return "width: the coarsest level is too small for one window and its ring";
    if (height < window + 3) return "height: the coarsest level is too small for one window and its ring";
    return nullptr;
}

extern "C" int dsdtm_klt_model_create(dsdtm_klt_ctx* ctx, int width, int height, int levels, dsdtm_klt_model** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "klt_model_create: out is NULL"); return DSDTM_ERR_INVALID; }
    if (levels == 0) levels = DSDTM_KLT_LEVELS;
    if (const char* bad = check_pyramid(width, height, levels, DSDTM_KLT_WINDOW)) { set_err(ctx, "klt_model_create: %s (%d x %d, %d levels)", bad, width, height, levels); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    dsdtm_klt_model* m = new (std::nothrow) dsdtm_klt_model();
    if (!m) return DSDTM_ERR_NOMEM;
    m->width = width; m->height = height; m->geom = make_geom(width, height, levels);
    void* p = nullptr;
    const size_t bytes = 2 * m->geom.bytes;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); delete m; set_err(ctx, "klt_model_create: hipMalloc of %zu bytes failed", bytes); return DSDTM_ERR_NOMEM; }
    m->pyr[0] = (uint8_t*)p; m->pyr[1] = (uint8_t*)p + m->geom.bytes;
    *out = m;
    return DSDTM_OK;
}

extern "C" void dsdtm_klt_model_destroy(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model) {
    if (!model) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }      // (a step's launches may still read it)
    if (model->pyr[0]) (void)hipFree(model->pyr[0]);
    delete model;
}

extern "C" int dsdtm_klt_model_reset(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!model) { set_err(ctx, "klt_model_reset: model is NULL"); return DSDTM_ERR_INVALID; }
    model->frames = 0;
    for (int i = 0; i < 9; ++i) model->H[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return DSDTM_OK;
}

extern "C" int dsdtm_klt_model_pyramid(dsdtm_klt_ctx* ctx, const dsdtm_klt_model* model, int level, uint8_t* dst, int dst_stride) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!model) { set_err(ctx, "klt_model_pyramid: model is NULL"); return DSDTM_ERR_INVALID; }
    if (model->frames == 0) { set_err(ctx, "klt_model_pyramid: the model has seen no image"); return DSDTM_ERR_INVALID; }
    if (level < 0 || level >= model->geom.levels) { set_err(ctx, "klt_model_pyramid: level %d outside 0..%d", level, model->geom.levels - 1); return DSDTM_ERR_INVALID; }
    if (!dst) { set_err(ctx, "klt_model_pyramid: dst is NULL"); return DSDTM_ERR_INVALID; }
    if (dst_stride < model->geom.w[level]) { set_err(ctx, "klt_model_pyramid: dst_stride is smaller than the level's width"); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy2DAsync(dst, (size_t)dst_stride, model->pyr[model->cur] + model->geom.off[level], (size_t)model->geom.stride[level],
                                  (size_t)model->geom.w[level], (size_t)model->geom.h[level], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DSDTM_OK;
}

// level 0 is in place: the other levels of one packed pyramid
static hipError_t build_levels(uint8_t* pyr, const Geom& g, hipStream_t stream) {
    for (int l = 0; l + 1 < g.levels; ++l) {
        const hipError_t e = pyrdown_launch(pyr, g.bytes, 1, g.w[l], g.h[l], g.stride[l], g.off[l], g.stride[l + 1], g.off[l + 1], stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

extern "C" int dsdtm_klt_steps(dsdtm_klt_ctx* ctx, int n, const dsdtm_klt_desc* descs, dsdtm_klt_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_KLT_MAX_STEPS) { set_err(ctx, "klt_steps: n = %d outside 0..%d", n, DSDTM_KLT_MAX_STEPS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "klt_steps: descs is NULL"); return DSDTM_ERR_INVALID; }
    if (!results) { set_err(ctx, "klt_steps: results is NULL"); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "klt_steps: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   LK records | ingest records | compaction records | homography records | grids | host images (pitch = width up to 16)
    //   || n_tracked | homography results | per model that asked: points, status, iterations, mask || the same of the others, a, b
    const size_t N = (size_t)n;
    struct Plan { int np = 0, gw = 0, gh = 0, mem = 0; bool first = false, back = false; size_t grid = 0, img = 0, pts = 0, st = 0, it = 0, mask = 0, a = 0, b = 0; };
    std::vector<Plan> plan(N);
    std::vector<const dsdtm_klt_model*> seen;
    seen.reserve(N);
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_desc& d = descs[t];
        Plan& p = plan[(size_t)t];
        const char* bad = nullptr;
        if (!d.model) bad = "model is NULL";
        else if (!d.image) bad = "image is NULL";
        else if (d.stride < d.model->width) bad = "stride is smaller than the width";
        else if (d.grid_w < 0 || d.grid_h < 0) bad = "grid_w / grid_h is negative";
        if (bad) { set_err(ctx, "klt_steps: step %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        p.gw = d.grid_w ? d.grid_w : 32; p.gh = d.grid_h ? d.grid_h : 24;
        p.np = grid_count(d.model->width, d.model->height, p.gw, p.gh);
        if (p.np > DSDTM_HOMOGRAPHY_MAX_POINTS) { set_err(ctx, "klt_steps: step %d: grid_w / grid_h give %d points, more than %d", t, p.np, DSDTM_HOMOGRAPHY_MAX_POINTS); return DSDTM_ERR_INVALID; }
        if (std::find(seen.begin(), seen.end(), d.model) != seen.end()) { set_err(ctx, "klt_steps: step %d: model appears twice in one call", t); return DSDTM_ERR_INVALID; }
        seen.push_back(d.model);
        p.mem = image_memory(ctx, d.image);
        if (p.mem < 0) { set_err(ctx, "klt_steps: step %d: image lies in another device's memory", t); return DSDTM_ERR_INVALID; }
        p.first = d.model->frames == 0;
        p.back = d.points || d.status || d.iterations || d.mask;
    }
    size_t o = 0;
    const size_t lk_at = o; o = align_up(o + N * sizeof(KltDev), 256);
    const size_t in_at = o; o = align_up(o + N * sizeof(KltIngest), 256);
    const size_t co_at = o; o = align_up(o + N * sizeof(KltCompact), 256);
    const size_t ho_at = o; o = align_up(o + N * sizeof(HomographyDev), 256);
    for (int t = 0; t < n; ++t) { plan[(size_t)t].grid = o; o += align_up((size_t)plan[(size_t)t].np * 8, 16); }
    for (int t = 0; t < n; ++t)
        if (plan[(size_t)t].mem == 0) { plan[(size_t)t].img = o; o += align_up((size_t)descs[t].model->width, 16) * (size_t)descs[t].model->height; }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t back_begin = o;
    const size_t nt_at = o; o = align_up(o + N * sizeof(int32_t), 16);
    const size_t hr_at = o; o = align_up(o + N * sizeof(dsdtm_homography_result), 16);
    auto place = [&](Plan& p) {
        const size_t np = (size_t)p.np;
        p.pts = o; o += align_up(np * 8, 16);
        p.st = o; o += align_up(np, 16);
        p.it = o; o += align_up(np * 4, 16);
        p.mask = o; o += align_up(np, 16);
    };
    for (Plan& p : plan) if (p.back) place(p);
    const size_t back_end = o;
    for (Plan& p : plan) if (!p.back) place(p);
    for (Plan& p : plan) { p.a = o; o += align_up((size_t)p.np * 8, 16); p.b = o; o += align_up((size_t)p.np * 8, 16); }
    if (int rc = ensure_stage(ctx, back_end, o)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    int max_points = 0, max_w = 0, max_h = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_desc& d = descs[t];
        const dsdtm_klt_model* m = d.model;
        const Plan& p = plan[(size_t)t];
        float* grid = (float*)(h + p.grid);
        int k = 0;
        for (int i = 0; i < m->width / p.gw - 1; ++i)
            for (int j = 0; j < m->height / p.gh - 1; ++j, ++k) { grid[2 * k] = (float)(i * p.gw + p.gw / 2); grid[2 * k + 1] = (float)(j * p.gh + p.gh / 2); }
        uint8_t* spare = m->pyr[1 - m->cur];
        KltIngest in;
        memset(&in, 0, sizeof in);
        in.dst = spare; in.width = m->width; in.height = m->height; in.dstride = m->geom.stride[0];
        if (p.mem == 0) {
            const size_t pitch = align_up((size_t)m->width, 16);
            for (int y = 0; y < m->height; ++y) memcpy(h + p.img + (size_t)y * pitch, d.image + (size_t)y * (size_t)d.stride, (size_t)m->width);
            in.src = g + p.img; in.sstride = (int32_t)pitch;
        } else { in.src = d.image; in.sstride = d.stride; }
        memcpy(h + in_at + (size_t)t * sizeof in, &in, sizeof in);
        KltDev r;
        memset(&r, 0, sizeof r);
        fill_dev(r, m->geom);
        r.prev = m->pyr[m->cur]; r.cur = spare;
        r.points = (const float*)(g + p.grid); r.guesses = nullptr;
        r.out_points = (float*)(g + p.pts); r.status = g + p.st; r.iterations = (int32_t*)(g + p.it); r.residual = nullptr;
        r.eps2 = DSDTM_KLT_EPSILON * DSDTM_KLT_EPSILON; r.min_eig = DSDTM_KLT_MIN_EIG;
        r.n_points = p.first ? 0 : p.np; r.window = DSDTM_KLT_WINDOW; r.max_iter = DSDTM_KLT_ITERATIONS;
        memcpy(h + lk_at + (size_t)t * sizeof r, &r, sizeof r);
        HomographyDev hr;
        memset(&hr, 0, sizeof hr);
        hr.a = (const float*)(g + p.a); hr.b = (const float*)(g + p.b); hr.mask = g + p.mask;
        hr.out = (dsdtm_homography_result*)(g + hr_at) + t;
        hr.thr2 = DSDTM_KLT_RANSAC_THRESHOLD * DSDTM_KLT_RANSAC_THRESHOLD;
        hr.left = 1.0 - DSDTM_HOMOGRAPHY_DEFAULT_CONFIDENCE;
        hr.m = 0;                                                    // (the compaction launch writes it)
        hr.rounds_max = (DSDTM_HOMOGRAPHY_DEFAULT_HYPOTHESES + HOMOGRAPHY_ROUND - 1) / HOMOGRAPHY_ROUND;
        hr.seed = DSDTM_HOMOGRAPHY_DEFAULT_SEED;
        memcpy(h + ho_at + (size_t)t * sizeof hr, &hr, sizeof hr);
        KltCompact c;
        memset(&c, 0, sizeof c);
        c.prev_points = r.points; c.points = r.out_points; c.status = r.status; c.a = (float*)(g + p.a); c.b = (float*)(g + p.b);
        c.rec = (HomographyDev*)(g + ho_at) + t; c.n_tracked = (int32_t*)(g + nt_at) + t;
        c.n_points = p.first ? 0 : p.np; c.min_tracked = DSDTM_KLT_MIN_TRACKED;
        memcpy(h + co_at + (size_t)t * sizeof c, &c, sizeof c);
        max_points = std::max(max_points, r.n_points); max_w = std::max(max_w, m->width); max_h = std::max(max_h, m->height);
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(klt_ingest_launch((const KltIngest*)(g + in_at), n, max_w, max_h, ctx->stream));
    for (int t = 0; t < n; ++t) API_TRY(build_levels(descs[t].model->pyr[1 - descs[t].model->cur], descs[t].model->geom, ctx->stream));
    API_TRY(klt_launch((const KltDev*)(g + lk_at), n, max_points, ctx->stream));
    API_TRY(klt_compact_launch((const KltCompact*)(g + co_at), n, ctx->stream));
    API_TRY(homography_launch((const HomographyDev*)(g + ho_at), n, ctx->stream));
    API_TRY(hipMemcpyAsync(h + back_begin, g + back_begin, back_end - back_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_desc& d = descs[t];
        dsdtm_klt_model* m = d.model;
        const Plan& p = plan[(size_t)t];
        int32_t nt = 0;
        memcpy(&nt, h + nt_at + (size_t)t * sizeof nt, sizeof nt);
        dsdtm_homography_result got;
        memcpy(&got, h + hr_at + (size_t)t * sizeof got, sizeof got);
        dsdtm_klt_result res;
        memset(&res, 0, sizeof res);
        res.n_points = p.np; res.n_tracked = nt; res.frame = m->frames;
        if (nt < DSDTM_KLT_MIN_TRACKED) { res.source = DSDTM_KLT_SOURCE_IDENTITY; res.H[0] = res.H[4] = res.H[8] = 1.0; }
        else if (got.found == 1) {
            res.source = DSDTM_KLT_SOURCE_RANSAC;
            memcpy(res.H, got.H, sizeof res.H);
            res.cost_before = got.cost_before; res.cost_after = got.cost_after; res.n_inliers = got.n_inliers;
            res.best_hypothesis = got.best_hypothesis; res.rounds = got.rounds; res.refit_iterations = got.refit_iterations;
        } else { res.source = DSDTM_KLT_SOURCE_KEPT; memcpy(res.H, m->H, sizeof res.H); }
        results[t] = res;
        const size_t np = (size_t)p.np;
        if (d.prev_points && np) memcpy(d.prev_points, h + p.grid, np * 8);
        if (p.first) {
            if (d.points && np) memcpy(d.points, h + p.grid, np * 8);
            if (d.status && np) memset(d.status, 0, np);
            if (d.iterations && np) memset(d.iterations, 0, np * 4);
        } else {
            if (d.points && np) memcpy(d.points, h + p.pts, np * 8);
            if (d.status && np) memcpy(d.status, h + p.st, np);
            if (d.iterations && np) memcpy(d.iterations, h + p.it, np * 4);
            if (d.mask && res.source == DSDTM_KLT_SOURCE_RANSAC) memcpy(d.mask, h + p.mask, (size_t)nt);
        }
        memcpy(m->H, res.H, sizeof m->H);
        m->cur = 1 - m->cur;                    // the swap: the current pyramid is the next step's previous one
        m->frames += 1;
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_klt_step(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model, const uint8_t* image, int stride, dsdtm_klt_result* result) {
    dsdtm_klt_desc d;
    memset(&d, 0, sizeof d);
    d.model = model; d.image = image; d.stride = stride;
    return dsdtm_klt_steps(ctx, 1, &d, result);
}

extern "C" int dsdtm_klt_flow(dsdtm_klt_ctx* ctx, int n, const dsdtm_klt_flow_desc* descs) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_KLT_MAX_STEPS) { set_err(ctx, "klt_flow: n = %d outside 0..%d", n, DSDTM_KLT_MAX_STEPS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "klt_flow: descs is NULL"); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "klt_flow: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    // the block's layout: LK records | ingest records (two per pair) | points, guesses | host images || out_points, status, iterations,
    // residual || the pyramids (two per pair)
    const size_t N = (size_t)n;
    struct Plan { Geom geom; int window = 0, levels = 0, iters = 0, mem[2] = {0, 0}; double eps = 0, min_eig = 0; size_t pts = 0, gs = 0, img[2] = {0, 0}, out = 0, st = 0, it = 0, res = 0, pyr[2] = {0, 0}; };
    std::vector<Plan> plan(N);
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_flow_desc& d = descs[t];
        Plan& p = plan[(size_t)t];
        p.window = d.window ? d.window : DSDTM_KLT_WINDOW; p.levels = d.levels ? d.levels : DSDTM_KLT_LEVELS;
        p.iters = d.iterations ? d.iterations : DSDTM_KLT_ITERATIONS;
        p.eps = d.epsilon != 0.0 ? d.epsilon : DSDTM_KLT_EPSILON; p.min_eig = d.min_eig != 0.0 ? d.min_eig : DSDTM_KLT_MIN_EIG;
        const char* bad = nullptr;
        if (!d.prev) bad = "prev is NULL";
        else if (!d.cur) bad = "cur is NULL";
        else if (d.n_points < 0 || d.n_points > DSDTM_KLT_MAX_FLOW_POINTS) bad = "n_points out of range";
        else if (d.n_points > 0 && !d.points) bad = "points is NULL";
        else if (d.n_points > 0 && !d.out_points) bad = "out_points is NULL";
        else if (p.iters < 1 || p.iters > 100) bad = "iterations outside 1..100";
        else if (!std::isfinite(p.eps) || p.eps < 0.0) bad = "epsilon is negative or not finite";
        else if (!std::isfinite(p.min_eig) || p.min_eig < 0.0) bad = "min_eig is negative or not finite";
        else bad = check_pyramid(d.width, d.height, p.levels, p.window);
        if (!bad && (d.prev_stride < d.width)) bad = "prev_stride is smaller than the width";
        if (!bad && (d.cur_stride < d.width)) bad = "cur_stride is smaller than the width";
        if (bad) { set_err(ctx, "klt_flow: pair %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        for (int i = 0; i < 2 * d.n_points; ++i) {
            if (!std::isfinite(d.points[i]) || std::fabs(d.points[i]) > 1.0e5f) { set_err(ctx, "klt_flow: pair %d: points is not finite or beyond 1e5 at index %d", t, i / 2); return DSDTM_ERR_INVALID; }
            if (d.guesses && (!std::isfinite(d.guesses[i]) || std::fabs(d.guesses[i]) > 1.0e5f)) { set_err(ctx, "klt_flow: pair %d: guesses is not finite or beyond 1e5 at index %d", t, i / 2); return DSDTM_ERR_INVALID; }
        }
        p.mem[0] = image_memory(ctx, d.prev); p.mem[1] = image_memory(ctx, d.cur);
        if (p.mem[0] < 0 || p.mem[1] < 0) { set_err(ctx, "klt_flow: pair %d: an image lies in another device's memory", t); return DSDTM_ERR_INVALID; }
        p.geom = make_geom(d.width, d.height, p.levels);
    }
    size_t o = 0;
    const size_t lk_at = o; o = align_up(o + N * sizeof(KltDev), 256);
    const size_t in_at = o; o = align_up(o + 2 * N * sizeof(KltIngest), 256);
    for (int t = 0; t < n; ++t) {
        Plan& p = plan[(size_t)t];
        const size_t np = (size_t)descs[t].n_points;
        p.pts = o; o += align_up(np * 8, 16);
        if (descs[t].guesses) { p.gs = o; o += align_up(np * 8, 16); }
        for (int s = 0; s < 2; ++s)
            if (p.mem[s] == 0) { p.img[s] = o; o += align_up((size_t)descs[t].width, 16) * (size_t)descs[t].height; }
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t back_begin = o;
    for (int t = 0; t < n; ++t) {
        Plan& p = plan[(size_t)t];
        const size_t np = (size_t)descs[t].n_points;
        p.out = o; o += align_up(np * 8, 16);
        p.st = o; o += align_up(np, 16);
        p.it = o; o += align_up(np * 4, 16);
        p.res = o; o += align_up(np * 4, 16);
    }
    const size_t back_end = o;
    for (Plan& p : plan) for (int s = 0; s < 2; ++s) { o = align_up(o, 256); p.pyr[s] = o; o += p.geom.bytes; }
    if (int rc = ensure_stage(ctx, back_end, o)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    int max_points = 0, max_w = 0, max_h = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_flow_desc& d = descs[t];
        const Plan& p = plan[(size_t)t];
        const size_t np = (size_t)d.n_points;
        if (np) memcpy(h + p.pts, d.points, np * 8);
        if (np && d.guesses) memcpy(h + p.gs, d.guesses, np * 8);
        for (int s = 0; s < 2; ++s) {
            const uint8_t* src = s ? d.cur : d.prev;
            const int sstride = s ? d.cur_stride : d.prev_stride;
            KltIngest in;
            memset(&in, 0, sizeof in);
            in.dst = g + p.pyr[s]; in.width = d.width; in.height = d.height; in.dstride = p.geom.stride[0];
            if (p.mem[s] == 0) {
                const size_t pitch = align_up((size_t)d.width, 16);
                for (int y = 0; y < d.height; ++y) memcpy(h + p.img[s] + (size_t)y * pitch, src + (size_t)y * (size_t)sstride, (size_t)d.width);
                in.src = g + p.img[s]; in.sstride = (int32_t)pitch;
            } else { in.src = src; in.sstride = sstride; }
            memcpy(h + in_at + (2 * (size_t)t + (size_t)s) * sizeof in, &in, sizeof in);
        }
        KltDev r;
        memset(&r, 0, sizeof r);
        fill_dev(r, p.geom);
        r.prev = g + p.pyr[0]; r.cur = g + p.pyr[1];
        r.points = (const float*)(g + p.pts); r.guesses = d.guesses ? (const float*)(g + p.gs) : nullptr;
        r.out_points = (float*)(g + p.out); r.status = g + p.st; r.iterations = (int32_t*)(g + p.it); r.residual = (float*)(g + p.res);
        r.eps2 = p.eps * p.eps; r.min_eig = p.min_eig;
        r.n_points = d.n_points; r.window = p.window; r.max_iter = p.iters;
        memcpy(h + lk_at + (size_t)t * sizeof r, &r, sizeof r);
        max_points = std::max(max_points, d.n_points); max_w = std::max(max_w, d.width); max_h = std::max(max_h, d.height);
    }
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(klt_ingest_launch((const KltIngest*)(g + in_at), 2 * n, max_w, max_h, ctx->stream));
    for (const Plan& p : plan) for (int s = 0; s < 2; ++s) API_TRY(build_levels(g + p.pyr[s], p.geom, ctx->stream));
    API_TRY(klt_launch((const KltDev*)(g + lk_at), n, max_points, ctx->stream));
    if (back_end > back_begin) API_TRY(hipMemcpyAsync(h + back_begin, g + back_begin, back_end - back_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const dsdtm_klt_flow_desc& d = descs[t];
        const Plan& p = plan[(size_t)t];
        const size_t np = (size_t)d.n_points;
        if (!np) continue;
        memcpy(d.out_points, h + p.out, np * 8);
        if (d.status) memcpy(d.status, h + p.st, np);
        if (d.iterations_used) memcpy(d.iterations_used, h + p.it, np * 4);
        if (d.residual) memcpy(d.residual, h + p.res, np * 4);
    }
    return DSDTM_OK;
}
