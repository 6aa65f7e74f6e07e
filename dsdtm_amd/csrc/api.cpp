// api.cpp — the C ABI of include/dsdtm_amd.h: context, host staging, launches (the tracked-frame entries: api_track.cpp; local BA: api_local_ba.cpp; shared: api_internal.h).
//
// Host entry points pack their inputs into one pinned buffer, move it with a single
// hipMemcpyAsync, launch on the context's stream and copy the (small) results back. Device
// entry points only enqueue kernels. There is no CPU compute path in this library.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "api_internal.h"

using namespace dsdtm;
using namespace dsdtm::detail;

// Contexts that are alive (dsdtm_frame_destroy may be handed a context that is already gone: it must not be dereferenced)
static std::mutex g_live_mutex;
static std::vector<dsdtm_ctx*> g_live_ctx;
static bool ctx_is_live_locked(dsdtm_ctx* ctx) {      // (g_live_mutex held)
    for (dsdtm_ctx* c : g_live_ctx) if (c == ctx) return true;
    return false;
}

static thread_local char g_create_err[512] = "";

void dsdtm::detail::set_err(dsdtm_ctx* ctx, const char* fmt, ...) {
    char* dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

// The packed pyramid of an image (Frame::ComputeImagePyramid: level l is ((w + 1) / 2, (h + 1) / 2) of level l - 1); st: the strides
void dsdtm::detail::plan_image_pyramid(int width, int height, int levels, PackedPyr* pl, int st[]) {
    pl->levels = levels;
    size_t o = 0;
    for (int l = 0; l < levels; ++l) {
        pl->w[l] = l ? (pl->w[l - 1] + 1) / 2 : width; pl->h[l] = l ? (pl->h[l - 1] + 1) / 2 : height; st[l] = pl->w[l];
        pl->off[l] = o; o += align_up((size_t)pl->w[l] * pl->h[l], 64);
    }
    pl->bytes = o;
}

static bool same_geometry(const PackedPyr& a, const PackedPyr& b) {
    return a.levels == b.levels && !memcmp(a.w, b.w, sizeof(int) * a.levels) && !memcmp(a.h, b.h, sizeof(int) * a.levels);
}

// Level l of a caller's level table lies inside `limit` bytes: it has pixels, its rows are no shorter than they are wide and its
// last row ends inside. lv (may be NULL: the check alone): the level as the kernels take it.
static bool level_fits(int l, const int* width, const int* height, const int* stride, const size_t* level_offset, size_t limit, LevelGeom* lv) {
    if (width[l] <= 0 || height[l] <= 0 || stride[l] < width[l] || level_offset[l] + (size_t)stride[l] * height[l] > limit) return false;
    if (lv) { lv[l].w = width[l]; lv[l].h = height[l]; lv[l].stride = stride[l]; lv[l].off = (uint32_t)level_offset[l]; }
    return true;
}
// ... for a whole table; the first level that does not fit is named in the message. who: the entry's prefix; inside: the limit in its words.
static int check_levels(dsdtm_ctx* ctx, int levels, const int* width, const int* height, const int* stride, const size_t* level_offset,
                        size_t limit, const char* who, const char* inside, LevelGeom* lv) {
    for (int l = 0; l < levels; ++l)
        if (!level_fits(l, width, height, stride, level_offset, limit, lv)) {
            set_err(ctx, "%slevel %d does not fit inside %s", who, l, inside); return DSDTM_ERR_INVALID;
        }
    return DSDTM_OK;
}

// The layout of a staging block: a column starts where the one before it ended, rounded up to its alignment (an empty column takes no room)
struct StageLayout {
    size_t off = 0;
    size_t take(size_t bytes, size_t align = 256) { const size_t o = off; off = align_up(off + bytes, align); return o; }
};

// behind a timeout word of `stream` (which has drained): a pair that was stopped may have left its counter word behind
void dsdtm::detail::clear_stream_counters(dsdtm_ctx* ctx, hipStream_t stream) {
    for (int i = 0; i < dsdtm_ctx::MAX_STREAMS; ++i)
        if (ctx->rings[i].used && ctx->rings[i].stream == stream)
            (void)hipMemset(ctx->d_counter + i * dsdtm_ctx::COUNTERS_PER_STREAM, 0, sizeof(unsigned) * dsdtm_ctx::COUNTERS_PER_STREAM);
}

// ---- diagnostic switches (kernels.h: Options) — diagnostic build only ----------------------------
// The release library has no switches: options() is a compile-time constant there, nothing reads the environment,
// and no dsdtm_debug_* symbol exists (tests/test_capi_cpu.py checks `nm -D` and `strings`).
#ifdef DSDTM_DIAG
namespace {
struct OptionKey { const char* key; const char* env; int dsdtm::Options::*field; bool flag; };
const OptionKey kOptionKeys[] = {
    {"no_team", "DSDTM_NO_TEAM", &dsdtm::Options::no_team, true},
    {"ws_no_duo", "DSDTM_WS_NO_DUO", &dsdtm::Options::ws_no_duo, true},
    {"ws_no_sort", "DSDTM_WS_NO_SORT", &dsdtm::Options::ws_no_sort, true},
    {"fmd_split", "DSDTM_FMD_SPLIT", &dsdtm::Options::fmd_split, true},
    {"fmd_no_xcd", "DSDTM_FMD_NO_XCD", &dsdtm::Options::fmd_no_xcd, true},
    {"pyr_fused", "DSDTM_PYR_FUSED", &dsdtm::Options::pyr_fused, false},
    {"pyr_band", "DSDTM_PYR_BAND", &dsdtm::Options::pyr_band, false},
    {"no_recover", "DSDTM_NO_RECOVER", &dsdtm::Options::no_recover, true},
    {"team_no_wrap_clear", "DSDTM_TEAM_NO_WRAP_CLEAR", &dsdtm::Options::team_no_wrap_clear, true},
};
std::once_flag g_options_once;
void options_from_env() {
    dsdtm::Options& o = dsdtm::options();
    for (const OptionKey& k : kOptionKeys)
        if (const char* v = getenv(k.env)) o.*(k.field) = k.flag ? 1 : atoi(v);    // a flag is set by its presence
}
}  // namespace
dsdtm::Options& dsdtm::options() {
    static Options o;
    return o;
}
#endif  // DSDTM_DIAG

extern "C" {

#ifdef DSDTM_DIAG
const char* dsdtm_version(void) { return "dsdtm_amd 0.6 (gfx950, HIP; FP64 reference grid; DIAGNOSTIC build)"; }
#else
const char* dsdtm_version(void) { return "dsdtm_amd 0.6 (gfx950, HIP; FP64 reference grid)"; }
#endif

int dsdtm_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return DSDTM_ERR_NO_DEVICE;
    return n;
}

const char* dsdtm_last_error(const dsdtm_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

int dsdtm_create(int device, dsdtm_ctx** out) {
    if (!out) return DSDTM_ERR_INVALID;
    *out = nullptr;
#ifdef DSDTM_DIAG
    std::call_once(g_options_once, options_from_env);     // diagnostic build: the only place the library reads the environment
#endif
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err(nullptr, "no HIP device visible (%s); dsdtm_amd has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return DSDTM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_err(nullptr, "device %d out of range (%d visible)", device, n);
        return DSDTM_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        set_err(nullptr, "hipGetDeviceProperties(%d) failed", device);
        return DSDTM_ERR_NO_DEVICE;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "device %d is %s; this library contains gfx950 (MI355X) code objects only", device,
                prop.gcnArchName);
        return DSDTM_ERR_NO_DEVICE;
    }
    dsdtm_ctx* ctx = new (std::nothrow) dsdtm_ctx();
    if (!ctx) return DSDTM_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        set_err(nullptr, "hipSetDevice/hipStreamCreate failed on device %d", device);
        delete ctx;
        return DSDTM_ERR_HIP;
    }
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        // The team / two-member kernels place the members of a pair on one XCD by workgroup number (b, b + 8, ...) and
        // rely on all 256 CUs being one partition: anything else (CPX/DPX/QPX modes, fewer XCDs) runs the one-CU kernels.
        int xccs = 0;
        if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) xccs = 0;
        ctx->multi_cu_ok = (xccs == 8 && ctx->num_cus == 256);
    }
    const size_t counter_bytes = sizeof(unsigned) * (dsdtm_ctx::MAX_STREAMS * dsdtm_ctx::COUNTERS_PER_STREAM + dsdtm_ctx::GRAPH_COUNTERS);
    void* hf = nullptr;
    void* hfd = nullptr;
    if (hipHostMalloc(&hf, sizeof(unsigned) * dsdtm_ctx::N_FLAGS, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(&hfd, hf, 0) == hipSuccess) {
        memset(hf, 0, sizeof(unsigned) * dsdtm_ctx::N_FLAGS);
        ctx->h_flags = (volatile unsigned*)hf; ctx->d_flags = (unsigned*)hfd;
    }
    if (!ctx->d_flags ||
        hipMalloc((void**)&ctx->d_counter, counter_bytes) != hipSuccess ||
        hipMalloc((void**)&ctx->d_team, 8 * sparse_align_team_bytes(64)) != hipSuccess ||
        hipMemset(ctx->d_counter, 0, counter_bytes) != hipSuccess ||
        hipMemset(ctx->d_team, 0, 8 * sparse_align_team_bytes(64)) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->team_event, hipEventDisableTiming) != hipSuccess) {
        if (ctx->d_counter) (void)hipFree(ctx->d_counter);
        if (ctx->d_team) (void)hipFree(ctx->d_team);
        if (hf) (void)hipHostFree(hf);
        set_err(nullptr, "hipMalloc failed on device %d", device);
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return DSDTM_ERR_NOMEM;
    }
    try {
        std::lock_guard<std::mutex> g(g_live_mutex);
        g_live_ctx.push_back(ctx);
    } catch (...) { dsdtm_destroy(ctx); return DSDTM_ERR_NOMEM; }
    *out = ctx;
    return DSDTM_OK;
}

#ifdef DSDTM_DIAG
// Diagnostic switches by name (tests, A/B tools): the keys of kOptionKeys, process-wide. Returns DSDTM_ERR_INVALID
// for an unknown key. Not for production use: no entry point synchronises against a concurrent change.
int dsdtm_debug_set_option(const char* key, int value) {
    std::call_once(g_options_once, options_from_env);
    for (const OptionKey& k : kOptionKeys)
        if (key && strcmp(key, k.key) == 0) { dsdtm::options().*(k.field) = value; return DSDTM_OK; }
    return DSDTM_ERR_INVALID;
}
int dsdtm_debug_get_option(const char* key, int* value) {
    std::call_once(g_options_once, options_from_env);
    for (const OptionKey& k : kOptionKeys)
        if (key && value && strcmp(key, k.key) == 0) { *value = dsdtm::options().*(k.field); return DSDTM_OK; }
    return DSDTM_ERR_INVALID;
}
#endif  // DSDTM_DIAG

void dsdtm_destroy(dsdtm_ctx* ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> g(g_live_mutex);
        for (size_t i = 0; i < g_live_ctx.size(); ++i)
            if (g_live_ctx[i] == ctx) { g_live_ctx.erase(g_live_ctx.begin() + (long)i); break; }
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->prefetch_stream) (void)hipStreamSynchronize(ctx->prefetch_stream);   // a prefetch may be pending: nothing is freed under it
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (ctx->prefetch_stream) (void)hipStreamDestroy(ctx->prefetch_stream);
    for (auto& e : ctx->prefetch_event) if (e) (void)hipEventDestroy(e);
    for (auto& sl : ctx->prefetch_slot) if (sl.h) (void)hipHostFree(sl.h);
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    if (ctx->d_ws) (void)hipFree(ctx->d_ws);
    for (auto& r : ctx->rings) { if (r.d_ws) (void)hipFree(r.d_ws); if (r.last) (void)hipEventDestroy(r.last); }
    if (ctx->d_counter) (void)hipFree(ctx->d_counter);
    if (ctx->d_team) (void)hipFree(ctx->d_team);
    if (ctx->team_event) (void)hipEventDestroy(ctx->team_event);
    for (auto& r : ctx->rec) { if (r.d_seed) (void)hipFree(r.d_seed); if (r.done) (void)hipEventDestroy(r.done); }
    for (auto& cs : ctx->copy_stream) if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    for (auto& e : ctx->copy_events) (void)hipEventDestroy(e);
    if (ctx->copy_fence) (void)hipEventDestroy(ctx->copy_fence);
    if (ctx->h_flags) (void)hipHostFree((void*)ctx->h_flags);
    for (auto& pf : ctx->frame_pool) (void)hipFree(pf.d);
    if (ctx->lba_event) { (void)hipEventSynchronize(ctx->lba_event); (void)hipEventDestroy(ctx->lba_event); }
    if (ctx->d_lba) (void)hipFree(ctx->d_lba);
    if (ctx->h_lba) (void)hipHostFree(ctx->h_lba);
    if (ctx->track_event) (void)hipEventDestroy(ctx->track_event);
    delete ctx;
}

}  // extern "C"

int dsdtm::detail::ensure_stage(dsdtm_ctx* ctx, size_t bytes) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes > ctx->h_cap) {
        if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
        ctx->h_pinned = nullptr; ctx->h_cap = 0;
        const size_t cap = align_up(bytes + bytes / 4, 1 << 16);
        HIP_TRY(ctx, hipHostMalloc(&ctx->h_pinned, cap, hipHostMallocDefault));
        ctx->h_cap = cap;
    }
    if (bytes > ctx->d_cap) {
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        ctx->d_stage = nullptr; ctx->d_cap = 0;
        const size_t cap = align_up(bytes + bytes / 4, 1 << 16);
        HIP_TRY(ctx, hipMalloc(&ctx->d_stage, cap));
        ctx->d_cap = cap;
    }
    return DSDTM_OK;
}

// The pinned staging block as the device addresses it (asked for at every call, as before: the block may have been regrown)
int dsdtm::detail::pinned_device_ptr(dsdtm_ctx* ctx, uint8_t** p) {
    void* hd = nullptr;
    HIP_TRY(ctx, hipHostGetDevicePointer(&hd, ctx->h_pinned, 0));
    *p = (uint8_t*)hd;
    return DSDTM_OK;
}

extern "C" int dsdtm_reserve(dsdtm_ctx* ctx, size_t workspace_bytes) {
    if (!ctx) return DSDTM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (workspace_bytes > ctx->ws_cap) {
        if (ctx->d_ws) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_ws); }
        ctx->d_ws = nullptr; ctx->ws_cap = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_ws, workspace_bytes));
        ctx->ws_cap = workspace_bytes;
    }
    return DSDTM_OK;
}

extern "C" size_t dsdtm_sparse_align_workspace_bytes(const dsdtm_batch_desc* b) {
    if (!b) return 0;
    return sparse_align_workspace_bytes(b->n_pairs, b->max_features);
}

int dsdtm::detail::validate_params(dsdtm_ctx* ctx, const dsdtm_align_params* p, int levels) {
    if (!p) { set_err(ctx, "params is NULL"); return DSDTM_ERR_INVALID; }
    if (p->max_level > levels || p->max_level > DSDTM_MAX_LEVELS || p->min_level < 0) {
        set_err(ctx, "level range [%d,%d) does not fit a %d-level pyramid", p->min_level, p->max_level, levels);
        return DSDTM_ERR_INVALID;
    }
    return DSDTM_OK;
}

// behind a launch that used ring entry `ring`: once every entry is taken, leave an event for a later hand-over
static int ring_mark_launch(dsdtm_ctx* ctx, int ring, hipStream_t stream) {
    if (ring < 0) return DSDTM_OK;
    bool full = true;
    for (const auto& r : ctx->rings) full = full && r.used;
    if (!full) return DSDTM_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->rings[ring].last, stream));
    ctx->rings[ring].last_recorded = true;
    return DSDTM_OK;
}

#ifdef DSDTM_DIAG
static thread_local void* g_stamp_out = nullptr;   // device buffer, set only by the stamps debug entry
static thread_local int g_team_drop_members = 0;         // set only by dsdtm_debug_sparse_align_short_team
#else
static constexpr void* g_stamp_out = nullptr;      // (release build: neither diagnostic exists)
static constexpr int g_team_drop_members = 0;
#endif

static int recover_settle(dsdtm_ctx* ctx, int slot, hipStream_t rerun_stream);
// Drops the re-run records of `stream` without settling them: for entry points that return an error and whose device
// buffers (the records hold raw pointers into them) may be freed or regrown before the next check on that stream.
static void recover_forget_stream(dsdtm_ctx* ctx, hipStream_t stream) {
    for (int i = 0; i < dsdtm_ctx::RECOVER_SLOTS; ++i)
        if (ctx->rec[i].used && ctx->rec[i].stream == stream) {
            ctx->rec[i].used = false;
            ctx->h_flags[dsdtm_ctx::FLAG_RECOVER + i] = 0;
        }
}

extern "C" int dsdtm_sparse_align_batch_device(dsdtm_ctx* ctx, const dsdtm_batch_desc* b, const dsdtm_camera* cam,
                                               const dsdtm_align_params* prm, void* hip_stream) {
    return launch_batch(ctx, b, cam, prm, hip_stream, LaunchMode{}, nullptr);
}

// A free recovery slot. When all are taken, the oldest launch is settled first (its event is waited for; a launch
// that timed out is re-run on its own stream): at most RECOVER_SLOTS unchecked multi-CU launches are in flight.
static int recover_acquire(dsdtm_ctx* ctx, int* slot_out) {
    int oldest = -1;
    for (int i = 0; i < dsdtm_ctx::RECOVER_SLOTS; ++i) {
        if (!ctx->rec[i].used) { *slot_out = i; return DSDTM_OK; }
        if (oldest < 0 || ctx->rec[i].order < ctx->rec[oldest].order) oldest = i;
    }
    // (settled on the stream it was launched on: a re-run must stay ordered with the later work queued there on the same
    // pose / count buffers; those buffers and the stream stay the caller's to keep alive until its check — dsdtm_amd.h)
    HIP_TRY(ctx, hipEventSynchronize(ctx->rec[oldest].done));
    if (int rc = recover_settle(ctx, oldest, ctx->rec[oldest].stream)) return rc;
    *slot_out = oldest;
    return DSDTM_OK;
}

// Settles slot `slot` (its launch has finished): forgotten when its timeout word is clear; otherwise the batch is
// re-seeded and re-run on the one-CU kernels on `rerun_stream`, which is then waited for.
static int recover_settle(dsdtm_ctx* ctx, int slot, hipStream_t rerun_stream) {
    dsdtm_ctx::Recover& r = ctx->rec[slot];
    if (!r.used) return DSDTM_OK;
    r.used = false;
    volatile unsigned* flag = ctx->h_flags + dsdtm_ctx::FLAG_RECOVER + slot;
    if (!*flag) return DSDTM_OK;
    *flag = 0;
    if (options().no_recover) {
        set_err(ctx, "sparse-align kernel: a wait for a partner workgroup timed out (re-run disabled: no_recover)");
        return DSDTM_ERR_HIP;
    }
    // The re-run is queued BEHIND whatever the caller issued on that stream since. A later unsettled launch of this stream that
    // names the same pose buffer (a loop into one buffer with no check in between) would have its results overwritten by this
    // older launch's: that cannot be repaired here, so it is reported instead of papered over (dsdtm_amd.h: unchecked launches
    // of one stream name distinct output buffers).
    for (int i = 0; i < dsdtm_ctx::RECOVER_SLOTS; ++i) {
        const dsdtm_ctx::Recover& y = ctx->rec[i];
        if (i != slot && y.used && y.stream == r.stream && y.order > r.order && y.b.T_cur_w == r.b.T_cur_w) {
            set_err(ctx, "sparse-align kernel: a wait for a partner workgroup timed out in a launch whose pose buffer a later unchecked "
                         "launch of the same stream reuses: it cannot be re-run (check the stream between launches into one buffer)");
            return DSDTM_ERR_HIP;
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(r.b.T_cur_w, r.d_seed, (size_t)r.b.n_pairs * 96, hipMemcpyDeviceToDevice, rerun_stream));
    LaunchMode m;
    m.one_cu = true;
    if (int rc = launch_batch(ctx, &r.b, &r.cam, &r.prm, rerun_stream, m, nullptr)) return rc;
    ctx->recovered += 1;
    return dsdtm_sparse_align_check(ctx, rerun_stream);
}

int dsdtm::detail::launch_batch(dsdtm_ctx* ctx, const dsdtm_batch_desc* b, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                                void* hip_stream, const LaunchMode& mode, bool* multi_cu_used) {
    if (multi_cu_used) *multi_cu_used = false;
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!b || !cam) { set_err(ctx, "batch/cam is NULL"); return DSDTM_ERR_INVALID; }
    if (int rc = validate_params(ctx, prm, b->levels)) return rc;
    if (b->n_pairs < 0 || b->max_features < 0 || b->max_features > 32767 || b->levels <= 0 || b->levels > DSDTM_MAX_LEVELS) {
        set_err(ctx, "bad batch geometry"); return DSDTM_ERR_INVALID;
    }
    if (b->n_pairs == 0) return DSDTM_OK;
    if (!b->ref_pyr || !b->cur_pyr || !b->T_ref_w || !b->T_cur_w || !b->n_tracked ||
        (b->max_features > 0 && (!b->px_xy || !b->bearing || !b->p_world || !b->initial))) {
        set_err(ctx, "batch descriptor has NULL device pointers"); return DSDTM_ERR_INVALID;
    }
    if ((b->pyr_pitch & 3) || b->pyr_pitch == 0 || b->pyr_pitch > 0xffffffffull ||
        (((size_t)b->ref_pyr) & 3) || (((size_t)b->cur_pyr) & 3)) {
        set_err(ctx, "pyramid base/pitch must be 4-byte aligned and pitch < 4 GiB"); return DSDTM_ERR_INVALID;
    }
    SAKernelArgs a;
    memset(&a, 0, sizeof a);
    if (int rc = check_levels(ctx, b->levels, b->width, b->height, b->stride, b->level_offset, b->pyr_pitch, "", "pyr_pitch", a.lv)) return rc;
    a.ref_pyr = b->ref_pyr; a.cur_pyr = b->cur_pyr; a.px_xy = b->px_xy; a.bearing = b->bearing;
    a.p_world = b->p_world; a.initial = b->initial; a.n_features = b->n_features;
    a.T_ref_w = b->T_ref_w; a.T_cur_w = b->T_cur_w; a.n_tracked = b->n_tracked; a.stats = b->stats;
    a.pyr_pitch = b->pyr_pitch; a.n_pairs = b->n_pairs; a.max_features = b->max_features;
    a.max_level = prm->max_level; a.min_level = prm->min_level; a.max_iters = prm->max_iters; a.min_fts = prm->min_fts;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.f = cam->f;
    a.ws_sort = options().ws_no_sort ? 0 : 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    int ring = -1;                                     // this stream's entry of ctx->rings (not while capturing)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    // the word the launch's persistent slots pull pair indices from (see dsdtm_ctx::d_counter)
    if (capturing) {
        if (ctx->graph_counters_used >= dsdtm_ctx::GRAPH_COUNTERS) {
            set_err(ctx, "more than %d launches captured into hipGraphs through one context: create another context",
                    dsdtm_ctx::GRAPH_COUNTERS);
            return DSDTM_ERR_INVALID;
        }
        a.pair_counter = ctx->d_counter + dsdtm_ctx::MAX_STREAMS * dsdtm_ctx::COUNTERS_PER_STREAM + ctx->graph_counters_used++;
        HIP_TRY(ctx, hipMemsetAsync(a.pair_counter, 0, sizeof(unsigned), stream));   // memset node: replays heal themselves
        a.timeout_flag = ctx->d_flags + dsdtm_ctx::FLAG_GRAPH;
    } else {
        int ri = -1;
        for (int i = 0; i < dsdtm_ctx::MAX_STREAMS && ri < 0; ++i)
            if (ctx->rings[i].used && ctx->rings[i].stream == stream) ri = i;
        for (int i = 0; i < dsdtm_ctx::MAX_STREAMS && ri < 0; ++i)
            if (!ctx->rings[i].used) {
                hipEvent_t ev = nullptr;
                HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                ctx->rings[i] = dsdtm_ctx::StreamRing{stream, 0u, true, nullptr, 0, 0ull, ev, false};
                ri = i;
            }
        if (ri < 0) {
            // A 17th stream (applications that keep creating streams): the entry that has been idle longest is handed
            // over once the launches behind it have finished — the host waits for the event recorded behind the
            // entry's last launch (an event outlives its stream; no device-wide synchronisation, which would also be
            // illegal while another stream is capturing). After that nothing uses the entry's counters or workspace.
            // Events are only recorded once all entries are taken (rings_full), so that applications with few
            // streams pay nothing; an entry last used before that is waited for with the device, once.
            ri = 0;
            for (int i = 1; i < dsdtm_ctx::MAX_STREAMS; ++i)
                if (ctx->rings[i].last_use < ctx->rings[ri].last_use) ri = i;
            if (ctx->rings[ri].last_recorded) HIP_TRY(ctx, hipEventSynchronize(ctx->rings[ri].last));
            else HIP_TRY(ctx, hipDeviceSynchronize());
            ctx->rings[ri].last_recorded = false;
            ctx->rings[ri].stream = stream;
            ctx->rings[ri].seq = 0;
            // (the previous owner's launches have drained: its word starts clean — a timeout it raised and nobody checked for
            // is not lost with it: the next check on any stream of this context reports it)
            if (ctx->h_flags[ri]) ctx->evicted_timeout = true;
            ctx->h_flags[ri] = 0;
        }
        ctx->rings[ri].last_use = ++ctx->ring_tick;
        a.pair_counter = ctx->d_counter + ri * dsdtm_ctx::COUNTERS_PER_STREAM + (ctx->rings[ri].seq++ % dsdtm_ctx::COUNTERS_PER_STREAM);
        ring = ri;
        a.timeout_flag = ctx->d_flags + ri;
    }
    if (mode.single) a.timeout_flag = ctx->d_flags + dsdtm_ctx::FLAG_SINGLE;
#ifdef DSDTM_DIAG
    if (g_stamp_out) {   // diagnostic path of dsdtm_debug_sparse_align_stamps
        if (b->max_features > 320) { set_err(ctx, "stamps: <=320 features only"); return DSDTM_ERR_INVALID; }
        a.workspace = (double*)g_stamp_out;
        HIP_TRY(ctx, sparse_align_launch_stamps(a, ctx->num_cus, stream));
        return DSDTM_OK;
    }
#endif
    // Few pairs of more than 448 features: one pair over K compute units. The members of a team spin on each
    // other, so all of a launch's workgroups must be resident together: sparse_align_team_size admits a launch
    // only when it fills at most half the CUs, and the team launches of a context are totally ordered — one on
    // another stream first waits for the previous one's event — so two of them never compete for CUs (kernels
    // of OTHER kinds on other streams can still delay a member: such a wait ends when their workgroups drain; a
    // wait that does not end raises the timeout flag, see dsdtm_sparse_align_check). Not used while capturing
    // (a graph replay could not be ordered against live team launches): those shapes take the one-CU kernels.
    // Multi-CU kernels only where their dispatch assumptions hold, never in a re-run, never while capturing (a graph
    // replay could neither be ordered against live team launches nor be re-run after a timeout).
    const bool multi_cu = ctx->multi_cu_ok && !mode.one_cu && !capturing;
    const int team_k = (multi_cu && b->n_pairs <= 64 && !options().no_team) ? sparse_align_team_size(b->n_pairs, b->max_features, ctx->num_cus) : 0;
    const SAVariant v = mode.variant >= 0 ? (SAVariant)mode.variant : sparse_align_pick_variant(b->max_features);
    const size_t ws = mode.variant >= 0 ? 0 : sparse_align_workspace_bytes(b->n_pairs, b->max_features);
    a.ref_ptrs = mode.ref_ptrs;
    a.cur_ptrs = mode.ref_ptrs ? mode.cur_ptrs : nullptr;
    const bool duo = !team_k && multi_cu && sparse_align_uses_duo(b->max_features, ws != 0);
    int slot = -1;
    if ((team_k || duo) && !mode.single) {
        // what a re-run needs, should a wait for a partner workgroup run out (dsdtm_ctx::Recover)
        if (int rc = recover_acquire(ctx, &slot)) return rc;
        dsdtm_ctx::Recover& r = ctx->rec[slot];
        const size_t seed_bytes = (size_t)b->n_pairs * 96;
        if (seed_bytes > r.seed_cap) {
            if (r.d_seed) (void)hipFree(r.d_seed);     // (the slot is free: nothing in flight uses its buffer)
            r.d_seed = nullptr; r.seed_cap = 0;
            HIP_TRY(ctx, hipMalloc(&r.d_seed, align_up(seed_bytes, 4096)));
            r.seed_cap = align_up(seed_bytes, 4096);
        }
        if (!r.done) HIP_TRY(ctx, hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
        HIP_TRY(ctx, hipMemcpyAsync(r.d_seed, b->T_cur_w, seed_bytes, hipMemcpyDeviceToDevice, stream));
        r.b = *b; r.cam = *cam; r.prm = *prm; r.stream = stream; r.order = ++ctx->rec_tick;
        ctx->h_flags[dsdtm_ctx::FLAG_RECOVER + slot] = 0;
        a.timeout_flag = ctx->d_flags + dsdtm_ctx::FLAG_RECOVER + slot;
    }
    if (multi_cu_used) *multi_cu_used = team_k || duo;
    auto launched_multi_cu = [&]() -> int {
        if (slot < 0) return DSDTM_OK;
        HIP_TRY(ctx, hipEventRecord(ctx->rec[slot].done, stream));
        ctx->rec[slot].used = true;
        return DSDTM_OK;
    };
    // Few pairs of more than 448 features: one pair over K compute units. The members of a team spin on each
    // other, so all of a launch's workgroups must be resident together: sparse_align_team_size admits a launch
    // only when it fills at most half the CUs, and the team launches of a context are totally ordered — one on
    // another stream first waits for the previous one's event — so two of them never compete for CUs (kernels
    // of OTHER kinds on other streams can still delay a member: such a wait ends when their workgroups drain; a
    // wait that does not end raises the launch's timeout word and the batch is re-run on the one-CU kernels, see
    // recover_settle).
    if (const int k = team_k) {
        if (ctx->team_any && ctx->team_last_stream != stream) {
            // the context's own stream is alive as long as the context: its event is recorded on demand;
            // launches on a caller's stream left theirs behind (that stream may be gone by now)
            if (ctx->team_last_stream == ctx->stream) HIP_TRY(ctx, hipEventRecord(ctx->team_event, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->team_event, 0));
        }
        // (the exchange words carry the launch's epoch in their tags — never 0, the buffers were zeroed when the context
        // was created — so a ring slot is reused without clearing it.) The tags hold 20 bits of epoch: ring slot and epoch
        // repeat together every 2^20 team launches, and a word that member m of pair p last wrote exactly then (team sizes
        // vary from frame to frame) would carry a tag this launch accepts. So when the epoch wraps, all eight ring slots
        // are zeroed on the launch stream — behind every earlier team launch (they are totally ordered, above) — once per
        // 2^20 launches; the reference's Run is stateless across calls (src/Sprase_ImageAlign.cpp:22-27).
        ctx->team_seq += 1;
        if ((ctx->team_seq & 0xfffffu) == 0u) {
            ctx->team_seq += 1;                           // epoch 0 = "never written"
            if (!options().team_no_wrap_clear)
                HIP_TRY(ctx, hipMemsetAsync(ctx->d_team, 0, 8 * sparse_align_team_bytes(64), stream));
            ctx->team_wraps += 1;
        }
        uint8_t* tslot = ctx->d_team + (size_t)(ctx->team_seq & 7u) * sparse_align_team_bytes(64);
        a.workspace = (double*)tslot;
        a.team_epoch = ctx->team_seq;
        if (g_team_drop_members) a.spin_limit = 1u << 12;      // the test's waits give up after ~4 k polls
        HIP_TRY(ctx, sparse_align_launch_team(a, k, stream, g_team_drop_members));
        if (int rc = launched_multi_cu()) return rc;
        if (int rc = ring_mark_launch(ctx, ring, stream)) return rc;
        if (stream != ctx->stream) HIP_TRY(ctx, hipEventRecord(ctx->team_event, stream));
        ctx->team_any = true; ctx->team_last_stream = stream;
        return DSDTM_OK;
    }
    if (ws) {
        // Scratch of the workspace kernel. A live launch uses its STREAM's workspace (the stream runs its launches
        // in order, so launches on different streams never share scratch; grown on demand, which synchronises that
        // stream once). A captured launch cannot allocate: it uses the context's reserved workspace (dsdtm_reserve),
        // which graph replays then share — replays of graphs captured through one context must not overlap.
        if (capturing) {
            if (ws > ctx->ws_cap) {
                set_err(ctx, "workspace of %zu bytes needed: call dsdtm_reserve before capturing", ws);
                return DSDTM_ERR_INVALID;
            }
            a.workspace = (double*)ctx->d_ws;
        } else {
            dsdtm_ctx::StreamRing& r = ctx->rings[ring];
            if (ws > r.ws_cap) {
                if (r.d_ws) { HIP_TRY(ctx, hipStreamSynchronize(stream)); (void)hipFree(r.d_ws); r.d_ws = nullptr; r.ws_cap = 0; }
                HIP_TRY(ctx, hipMalloc(&r.d_ws, ws));
                r.ws_cap = ws;
            }
            a.workspace = (double*)r.d_ws;
        }
    }
    if (duo && g_team_drop_members) { a.spin_limit = 1u << 12; a.debug_drop = 1; }    // tests: member 1 of every pair stays away
    HIP_TRY(ctx, sparse_align_launch(a, v, ctx->num_cus, stream, duo));
    if (int rc = launched_multi_cu()) return rc;
    return ring_mark_launch(ctx, ring, stream);
}

// Result check for callers of the asynchronous batch entry point: waits for `hip_stream`, then settles the launches
// issued on it since the last check. Multi-CU launches (team / two-member kernels) whose wait for a partner workgroup
// ran out are re-run on the one-CU kernels here — the caller sees DSDTM_OK and the results the reference's Run would
// have produced. DSDTM_ERR_HIP remains for a hand-over that failed INSIDE one workgroup (a broken protocol, never
// observed) or a re-run that failed too; the results of this stream's launches since the last check are then not to
// be trusted. Everything read here belongs to this context: no device-wide synchronisation, no device-global state.
extern "C" int dsdtm_sparse_align_check(dsdtm_ctx* ctx, void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    // this stream's multi-CU launches, in launch order (a re-run may feed a later launch of the same stream: the caller
    // sees final results only after this function returns)
    for (;;) {
        int next = -1;
        for (int i = 0; i < dsdtm_ctx::RECOVER_SLOTS; ++i)
            if (ctx->rec[i].used && ctx->rec[i].stream == stream && (next < 0 || ctx->rec[i].order < ctx->rec[next].order)) next = i;
        if (next < 0) break;
        if (int rc = recover_settle(ctx, next, stream)) return rc;
    }
    int ring = -1;
    for (int i = 0; i < dsdtm_ctx::MAX_STREAMS; ++i)
        if (ctx->rings[i].used && ctx->rings[i].stream == stream) ring = i;
    bool bad = false;
    if (ring >= 0 && ctx->h_flags[ring]) {
        ctx->h_flags[ring] = 0;
        // a pair that was stopped may have left its counter word behind: this stream's words (it has drained)
        (void)hipMemsetAsync(ctx->d_counter + ring * dsdtm_ctx::COUNTERS_PER_STREAM, 0, sizeof(unsigned) * dsdtm_ctx::COUNTERS_PER_STREAM, stream);
        (void)hipStreamSynchronize(stream);
        bad = true;
    }
    if (ctx->h_flags[dsdtm_ctx::FLAG_GRAPH]) { ctx->h_flags[dsdtm_ctx::FLAG_GRAPH] = 0; bad = true; }   // (graph launches zero their own counters)
    if (ctx->evicted_timeout) { ctx->evicted_timeout = false; bad = true; }
    if (bad) {
        set_err(ctx, "sparse-align kernel: a hand-over wait inside a workgroup timed out (results of this stream since the last check are invalid)");
        return DSDTM_ERR_HIP;
    }
    return DSDTM_OK;
}

#ifdef DSDTM_DIAG
extern "C" long long dsdtm_debug_recovered_launches(dsdtm_ctx* ctx) { return ctx ? (long long)ctx->recovered : -1; }
// Tests: the context's team-launch counter (its low 20 bits are the epoch of the exchange tags, its low 3 bits the ring slot),
// so that the epoch wrap — 2^20 team launches away in real use — can be crossed by a handful of launches. Returns the number
// of wraps seen so far. The caller's team launches must have drained.
extern "C" long long dsdtm_debug_team_seq(dsdtm_ctx* ctx, long long set_to) {
    if (!ctx) return -1;
    if (set_to >= 0) ctx->team_seq = (unsigned)set_to;
    return (long long)ctx->team_wraps;
}
#endif  // DSDTM_DIAG

// ---- the batch from host memory over several contexts / devices ------------------------------
extern "C" void dsdtm_shard_range(int n_pairs, int n_shards, int shard, int* lo, int* hi) {
    const int per = n_shards > 0 ? (n_pairs + n_shards - 1) / n_shards : n_pairs;
    int l = shard * per, h = l + per;
    if (l > n_pairs) l = n_pairs;
    if (h > n_pairs) h = n_pairs;
    if (n_pairs <= 0 || shard < 0 || shard >= n_shards) l = h = 0;
    if (lo) *lo = l;
    if (hi) *hi = h;
}

// The context's device staging alone, grown to `bytes` (never shrunk; what the context's stream still does with the old block is waited for)
static int ensure_device_stage(dsdtm_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->d_cap) return DSDTM_OK;
    if (ctx->d_stage) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_stage); }
    ctx->d_stage = nullptr; ctx->d_cap = 0;
    HIP_TRY(ctx, hipMalloc(&ctx->d_stage, bytes));
    ctx->d_cap = bytes;
    return DSDTM_OK;
}

// Where the columns of a staged batch start in its block (pair 0 of each; nf / st: only where has_nf / has_st)
struct BatchColumns { size_t ref, cur, px, be, pw, in, nf, tr, tc, nt, st; bool has_nf, has_st; };
// the columns of a shard of n pairs (n_ref reference pyramids; cur_in_ref: the current pyramids are the reference ones, shifted by one)
static BatchColumns plan_batch_columns(StageLayout& L, size_t n, size_t n_ref, bool cur_in_ref, size_t pit, size_t nf, bool has_nf, bool has_st) {
    BatchColumns c;
    c.ref = L.take(n_ref * pit); c.cur = cur_in_ref ? c.ref + pit : L.take(n * pit);
    c.px = L.take(n * nf * 8); c.be = L.take(n * nf * 24); c.pw = L.take(n * nf * 24); c.in = L.take(n * nf);
    c.nf = L.take(has_nf ? n * 4 : 0); c.tr = L.take(n * 96); c.tc = L.take(n * 96); c.nt = L.take(n * 4);
    c.st = L.take(has_st ? n * sizeof(dsdtm_align_stats) : 0);
    c.has_nf = has_nf; c.has_st = has_st;
    return c;
}
// b's pair count and columns: pairs [p0, p1) of the block at d (levels, pitch and max_features stay as they are)
static void bind_batch_columns(dsdtm_batch_desc& b, uint8_t* d, const BatchColumns& c, size_t pit, size_t nf, size_t p0, size_t p1) {
    b.n_pairs = (int)(p1 - p0);
    b.ref_pyr = d + c.ref + p0 * pit; b.cur_pyr = d + c.cur + p0 * pit;
    b.px_xy = (const float*)(d + c.px + p0 * nf * 8); b.bearing = (const double*)(d + c.be + p0 * nf * 24);
    b.p_world = (const double*)(d + c.pw + p0 * nf * 24); b.initial = d + c.in + p0 * nf;
    b.n_features = c.has_nf ? (const int32_t*)(d + c.nf + p0 * 4) : nullptr;
    b.T_ref_w = (const double*)(d + c.tr + p0 * 96); b.T_cur_w = (double*)(d + c.tc + p0 * 96);
    b.n_tracked = (int32_t*)(d + c.nt + p0 * 4);
    b.stats = c.has_st ? (dsdtm_align_stats*)(d + c.st + p0 * sizeof(dsdtm_align_stats)) : nullptr;
}
// the three result downloads of pairs [p0, p1) of the block into the caller's arrays, whose pair `first` is the block's pair 0
static int enqueue_result_downloads(dsdtm_ctx* ctx, double* T_cur_w, int32_t* n_tracked, dsdtm_align_stats* stats, size_t first, const uint8_t* d,
                                    const BatchColumns& c, size_t p0, size_t p1, hipStream_t st) {
    const size_t g0 = first + p0, np = p1 - p0;
    HIP_TRY(ctx, hipMemcpyAsync(T_cur_w + g0 * 12, d + c.tc + p0 * 96, np * 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(n_tracked + g0, d + c.nt + p0 * 4, np * 4, hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(ctx, hipMemcpyAsync(stats + g0, d + c.st + p0 * sizeof(dsdtm_align_stats), np * sizeof(dsdtm_align_stats), hipMemcpyDeviceToHost, st));
    return DSDTM_OK;
}

// One shard: pairs [lo, hi) of the host batch on `ctx` (its device, its stream). Device scratch comes from the
// context's staging buffer (device side only: the caller's arrays may be pageable, the copies are then staged by
// the runtime; pinned arrays are copied directly).
static int sharded_issue(dsdtm_ctx* ctx, const dsdtm_batch_desc* hb, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                         int lo, int hi) {
    const int n = hi - lo;
    if (n <= 0) return DSDTM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nf = (size_t)hb->max_features, pit = hb->pyr_pitch;
    StageLayout lay;
    const BatchColumns c = plan_batch_columns(lay, (size_t)n, (size_t)n, false, pit, nf, hb->n_features != nullptr, hb->stats != nullptr);
    if (int rc = ensure_device_stage(ctx, lay.off)) return rc;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    hipStream_t st = ctx->stream;
    auto up = [&](size_t o, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    HIP_TRY(ctx, up(c.ref, hb->ref_pyr + (size_t)lo * pit, n * pit));
    HIP_TRY(ctx, up(c.cur, hb->cur_pyr + (size_t)lo * pit, n * pit));
    HIP_TRY(ctx, up(c.px, hb->px_xy + (size_t)lo * nf * 2, n * nf * 8));
    HIP_TRY(ctx, up(c.be, hb->bearing + (size_t)lo * nf * 3, n * nf * 24));
    HIP_TRY(ctx, up(c.pw, hb->p_world + (size_t)lo * nf * 3, n * nf * 24));
    HIP_TRY(ctx, up(c.in, hb->initial + (size_t)lo * nf, n * nf));
    if (hb->n_features) HIP_TRY(ctx, up(c.nf, hb->n_features + lo, n * 4));
    HIP_TRY(ctx, up(c.tr, hb->T_ref_w + (size_t)lo * 12, n * 96));
    HIP_TRY(ctx, up(c.tc, hb->T_cur_w + (size_t)lo * 12, n * 96));
    dsdtm_batch_desc b = *hb;
    bind_batch_columns(b, d, c, pit, nf, 0, (size_t)n);
    if (int rc = dsdtm_sparse_align_batch_device(ctx, &b, cam, prm, st)) return rc;
    auto download = [&]() { return enqueue_result_downloads(ctx, hb->T_cur_w, hb->n_tracked, hb->stats, (size_t)lo, d, c, 0, (size_t)n, st); };
    // the downloads overlap nothing when queued before the check, but the check may re-seed and re-run a multi-CU launch whose
    // wait for a partner workgroup ran out (recover_settle): the host arrays then hold the aborted launch's poses and are
    // fetched again
    const unsigned long long rerun0 = ctx->recovered;
    if (int rc = download()) return rc;
    if (int rc = dsdtm_sparse_align_check(ctx, st)) return rc;
    if (ctx->recovered != rerun0) {
        if (int rc = download()) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return DSDTM_OK;
}

// The shard list of the two multi-context entries: no NULL context, no context twice (a context's stream and staging serve one shard)
static bool has_null_context(dsdtm_ctx* const* ctx, int n_ctx) {
    for (int g = 0; g < n_ctx; ++g) if (!ctx[g]) return true;
    return false;
}
static int check_distinct_contexts(dsdtm_ctx* const* ctx, int n_ctx, const char* who) {
    for (int g = 0; g < n_ctx; ++g)
        for (int h = g + 1; h < n_ctx; ++h)
            if (ctx[g] == ctx[h]) { set_err(ctx[0], "%s: a context appears twice (one context per shard)", who); return DSDTM_ERR_INVALID; }
    return DSDTM_OK;
}
// fn(g, lo, hi) for the shard of every context (dsdtm_shard_range over n_pairs): shards 1.. on a host thread each, shard 0 on the
// calling thread. Returns the first code that is not DSDTM_OK, in shard order. A shard whose thread cannot be started fails with
// DSDTM_ERR_NOMEM; no further shard is started then and shard 0 is not run.
template <class Fn>
static int run_shards(dsdtm_ctx* const* ctx, int n_ctx, int n_pairs, const char* who, Fn fn) {
    std::vector<int> rc(n_ctx, DSDTM_OK);
    std::vector<std::thread> th;
    bool spawn_failed = false;
    try { th.reserve((size_t)n_ctx); } catch (...) { set_err(ctx[0], "%s: out of memory", who); return DSDTM_ERR_NOMEM; }
    for (int g = 1; g < n_ctx && !spawn_failed; ++g) {
        int lo, hi;
        dsdtm_shard_range(n_pairs, n_ctx, g, &lo, &hi);
        try {
            th.emplace_back([=, &rc]() { rc[g] = fn(g, lo, hi); });
        } catch (...) {           // no exception crosses the C boundary: the shards already started are joined below
            spawn_failed = true;
            rc[g] = DSDTM_ERR_NOMEM;
            set_err(ctx[g], "%s: could not start the host thread of shard %d", who, g);
        }
    }
    if (!spawn_failed) {
        int lo, hi;
        dsdtm_shard_range(n_pairs, n_ctx, 0, &lo, &hi);
        rc[0] = fn(0, lo, hi);                                  // the calling thread takes the first shard
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < n_ctx; ++g) if (rc[g] != DSDTM_OK) return rc[g];
    return DSDTM_OK;
}

// A shard that fails half-way still has copies from / into the caller's arrays in flight: they are waited for before
// the error is returned, so the caller may free or reuse its memory as after any other return.
static int sharded_one(dsdtm_ctx* ctx, const dsdtm_batch_desc* hb, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                       int lo, int hi) {
    const int rc = sharded_issue(ctx, hb, cam, prm, lo, hi);
    if (rc != DSDTM_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        recover_forget_stream(ctx, ctx->stream);      // their records point into the staging buffer, which the next call may regrow
    }
    return rc;
}

extern "C" int dsdtm_sparse_align_batch_sharded(dsdtm_ctx* const* ctx, int n_ctx, const dsdtm_batch_desc* hb,
                                                const dsdtm_camera* cam, const dsdtm_align_params* prm) {
    if (!ctx || n_ctx <= 0 || !hb || !cam || !prm) return DSDTM_ERR_INVALID;
    if (has_null_context(ctx, n_ctx)) return DSDTM_ERR_INVALID;
    if (hb->n_pairs < 0 || !hb->ref_pyr || !hb->cur_pyr || !hb->T_ref_w || !hb->T_cur_w || !hb->n_tracked ||
        (hb->max_features > 0 && (!hb->px_xy || !hb->bearing || !hb->p_world || !hb->initial))) {
        set_err(ctx[0], "sharded batch: NULL host pointers"); return DSDTM_ERR_INVALID;
    }
    if (int rc = check_distinct_contexts(ctx, n_ctx, "sharded batch")) return rc;
    // the descriptor is checked BEFORE any shard sizes its staging from it or a thread is started
    if (hb->max_features < 0 || hb->max_features > 32767 || hb->levels <= 0 || hb->levels > DSDTM_MAX_LEVELS ||
        hb->pyr_pitch == 0 || (hb->pyr_pitch & 3) || hb->pyr_pitch > 0xffffffffull) {
        set_err(ctx[0], "sharded batch: bad geometry (max_features 0..32767, levels 1..%d, pyr_pitch a non-zero multiple of 4 below 4 GiB)",
                DSDTM_MAX_LEVELS);
        return DSDTM_ERR_INVALID;
    }
    if (int rc0 = validate_params(ctx[0], prm, hb->levels)) return rc0;
    if (int rc = check_levels(ctx[0], hb->levels, hb->width, hb->height, hb->stride, hb->level_offset, hb->pyr_pitch, "sharded batch: ", "pyr_pitch", nullptr)) return rc;
    return run_shards(ctx, n_ctx, hb->n_pairs, "sharded batch", [=](int g, int lo, int hi) { return sharded_one(ctx[g], hb, cam, prm, lo, hi); });
}

// ---- the batch STREAMED from host memory: level 0 only, chunked, copy overlapped with compute ---------------
// One shard = pairs [lo, hi) of the host sequence on `ctx`: chunks of `chunk` pairs; per chunk the level-0 images and
// feature columns go up on one of two copy streams, the pyramids are built by the device pyrDown and the chunk is
// aligned on the context's stream behind the copy's event, the results come back behind the alignment — the upload of
// chunk j + 1 overlaps pyramids + alignment + download of chunk j. Device memory holds the whole shard (0.41 MB per
// 640x480 frame: thousands of frames are a few GB of 288).
static int streamed_issue(dsdtm_ctx* ctx, const dsdtm_stream_desc* s, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                          int chunk, int lo, int hi) {
    const int n = hi - lo;
    if (n <= 0) return DSDTM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool chained = s->cur_image == nullptr;
    // device pyramid layout: the one dsdtm_frame_create_from_image uses (levels 64-byte aligned, pitch 256)
    PackedPyr pl;
    int st[DSDTM_MAX_LEVELS];
    plan_image_pyramid(s->width, s->height, s->levels, &pl, st);
    const size_t pit = align_up(pl.bytes, 256), img = (size_t)s->width * s->height, nf = (size_t)s->max_features;
    const int n_frames = chained ? n + 1 : n;
    StageLayout lay;
    const BatchColumns c = plan_batch_columns(lay, (size_t)n, (size_t)n_frames, chained, pit, nf, s->n_features != nullptr, s->stats != nullptr);
    if (int rc = ensure_device_stage(ctx, lay.off)) return rc;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    for (int i = 0; i < 2; ++i)
        if (!ctx->copy_stream[i]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream[i], hipStreamNonBlocking));
    const int n_chunks = (n + chunk - 1) / chunk;
    while ((int)ctx->copy_events.size() < n_chunks) {
        hipEvent_t e = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->copy_events.push_back(e);
    }
    // the copy streams start behind whatever the context's stream still does with the staging buffer
    if (!ctx->copy_fence) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->copy_fence, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ctx->copy_fence, ctx->stream));
    for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream[i], ctx->copy_fence, 0));
    // level 0 of frames [f0, f1) of host array `src` (frame 0 = the shard's first) -> device pyramids at d + base
    auto up_images = [&](hipStream_t cs, const uint8_t* src, size_t base, int f0, int f1) -> hipError_t {
        if (f1 <= f0) return hipSuccess;
        if (s->row_stride == s->width)      // whole images: ONE strided copy (an image is a "row" of W*H bytes)
            return hipMemcpy2DAsync(d + base + (size_t)f0 * pit, pit, src + (size_t)f0 * s->image_pitch, s->image_pitch, img,
                                    (size_t)(f1 - f0), hipMemcpyHostToDevice, cs);
        for (int f = f0; f < f1; ++f) {     // padded rows: one 2-D copy per image
            const hipError_t e = hipMemcpy2DAsync(d + base + (size_t)f * pit, (size_t)s->width, src + (size_t)f * s->image_pitch,
                                                  (size_t)s->row_stride, (size_t)s->width, (size_t)s->height, hipMemcpyHostToDevice, cs);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    auto up = [&](hipStream_t cs, size_t dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(d + dst, src, bytes, hipMemcpyHostToDevice, cs) : hipSuccess;
    };
    const uint8_t* ref_h = s->ref_image + (size_t)lo * s->image_pitch;
    const uint8_t* cur_h = chained ? nullptr : s->cur_image + (size_t)lo * s->image_pitch;
    dsdtm_batch_desc b;
    memset(&b, 0, sizeof b);
    b.max_features = s->max_features; b.pyr_pitch = pit;
    fill_levels(b, pl);
    hipStream_t comp = ctx->stream;
    for (int j = 0; j < n_chunks; ++j) {
        const int p0 = j * chunk, p1 = p0 + chunk < n ? p0 + chunk : n;      // pairs of this chunk (shard-relative)
        const size_t np = (size_t)(p1 - p0);
        hipStream_t cs = ctx->copy_stream[j & 1];
        // frames that arrive with this chunk — chained: the `cur` frames of its pairs (+ frame 0 with the first chunk)
        const int f0 = chained ? (j == 0 ? 0 : p0 + 1) : p0, f1 = chained ? p1 + 1 : p1;
        HIP_TRY(ctx, up_images(cs, ref_h, c.ref, f0, f1));
        if (!chained) HIP_TRY(ctx, up_images(cs, cur_h, c.cur, p0, p1));
        const size_t g0 = (size_t)(lo + p0);                                   // first pair of the chunk in the host arrays
        HIP_TRY(ctx, up(cs, c.px + p0 * nf * 8, s->px_xy + g0 * nf * 2, np * nf * 8));
        HIP_TRY(ctx, up(cs, c.be + p0 * nf * 24, s->bearing + g0 * nf * 3, np * nf * 24));
        HIP_TRY(ctx, up(cs, c.pw + p0 * nf * 24, s->p_world + g0 * nf * 3, np * nf * 24));
        HIP_TRY(ctx, up(cs, c.in + p0 * nf, s->initial + g0 * nf, np * nf));
        if (s->n_features) HIP_TRY(ctx, up(cs, c.nf + (size_t)p0 * 4, s->n_features + g0, np * 4));
        HIP_TRY(ctx, up(cs, c.tr + (size_t)p0 * 96, s->T_ref_w + g0 * 12, np * 96));
        HIP_TRY(ctx, up(cs, c.tc + (size_t)p0 * 96, s->T_cur_w + g0 * 12, np * 96));
        HIP_TRY(ctx, hipEventRecord(ctx->copy_events[j], cs));
        HIP_TRY(ctx, hipStreamWaitEvent(comp, ctx->copy_events[j], 0));
        // Frame::ComputeImagePyramid (src/Frame.cpp:74-81) for the frames that just arrived, on the device
        if (int rc = dsdtm_pyrdown_batch_device(ctx, d + c.ref + (size_t)f0 * pit, pit, f1 - f0, s->levels, pl.w, pl.h, st, pl.off, comp)) return rc;
        if (!chained)
            if (int rc = dsdtm_pyrdown_batch_device(ctx, d + c.cur + (size_t)p0 * pit, pit, p1 - p0, s->levels, pl.w, pl.h, st, pl.off, comp)) return rc;
        bind_batch_columns(b, d, c, pit, nf, (size_t)p0, (size_t)p1);
        if (int rc = dsdtm_sparse_align_batch_device(ctx, &b, cam, prm, comp)) return rc;
        // (multi-CU shapes: results are final after the check below; a chunk's download is repeated there if it was re-run)
        if (int rc = enqueue_result_downloads(ctx, s->T_cur_w, s->n_tracked, s->stats, (size_t)lo, d, c, (size_t)p0, (size_t)p1, comp)) return rc;
    }
    const unsigned long long rerun0 = ctx->recovered;
    if (int rc = dsdtm_sparse_align_check(ctx, comp)) return rc;
    if (ctx->recovered != rerun0) {          // a chunk was re-run on the one-CU kernels: fetch everything again
        if (int rc = enqueue_result_downloads(ctx, s->T_cur_w, s->n_tracked, s->stats, (size_t)lo, d, c, 0, (size_t)n, comp)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(comp));
    }
    return DSDTM_OK;
}

// As sharded_one: no copy touches the caller's arrays after an error return.
static int streamed_one(dsdtm_ctx* ctx, const dsdtm_stream_desc* s, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                        int chunk, int lo, int hi) {
    const int rc = streamed_issue(ctx, s, cam, prm, chunk, lo, hi);
    if (rc != DSDTM_OK) {
        for (int i = 0; i < 2; ++i)
            if (ctx->copy_stream[i]) (void)hipStreamSynchronize(ctx->copy_stream[i]);
        (void)hipStreamSynchronize(ctx->stream);
        recover_forget_stream(ctx, ctx->stream);      // as sharded_one
    }
    return rc;
}

extern "C" int dsdtm_sparse_align_batch_streamed(dsdtm_ctx* const* ctx, int n_ctx, const dsdtm_stream_desc* s, int chunk_pairs,
                                                 const dsdtm_camera* cam, const dsdtm_align_params* prm) {
    if (!ctx || n_ctx <= 0 || !s || !cam || !prm) return DSDTM_ERR_INVALID;
    if (has_null_context(ctx, n_ctx)) return DSDTM_ERR_INVALID;
    if (int rc = check_distinct_contexts(ctx, n_ctx, "streamed batch")) return rc;
    if (s->n_pairs < 0 || !s->ref_image || !s->T_ref_w || !s->T_cur_w || !s->n_tracked ||
        (s->max_features > 0 && (!s->px_xy || !s->bearing || !s->p_world || !s->initial))) {
        set_err(ctx[0], "streamed batch: NULL host pointers"); return DSDTM_ERR_INVALID;
    }
    if (s->max_features < 0 || s->max_features > 32767 || s->levels <= 0 || s->levels > DSDTM_MAX_LEVELS || s->width <= 0 ||
        s->height <= 0 || s->row_stride < s->width || s->image_pitch < (size_t)s->row_stride * (s->height - 1) + s->width) {
        set_err(ctx[0], "streamed batch: bad geometry"); return DSDTM_ERR_INVALID;
    }
    if (int rc0 = validate_params(ctx[0], prm, s->levels)) return rc0;
    const int chunk = chunk_pairs > 0 ? chunk_pairs : 128;
    return run_shards(ctx, n_ctx, s->n_pairs, "streamed batch", [=](int g, int lo, int hi) { return streamed_one(ctx[g], s, cam, prm, chunk, lo, hi); });
}

// ---- host staging helpers ---------------------------------------------------------------

static int plan_pyramid(dsdtm_ctx* ctx, const dsdtm_pyramid* p, PackedPyr* out) {
    if (!p || p->levels <= 0 || p->levels > DSDTM_MAX_LEVELS) { set_err(ctx, "bad pyramid"); return DSDTM_ERR_INVALID; }
    size_t off = 0;
    out->levels = p->levels;
    for (int l = 0; l < p->levels; ++l) {
        if (!p->data[l] || p->width[l] <= 0 || p->height[l] <= 0 || p->stride[l] < p->width[l]) {
            set_err(ctx, "bad pyramid level %d", l); return DSDTM_ERR_INVALID;
        }
        out->w[l] = p->width[l]; out->h[l] = p->height[l]; out->off[l] = off;
        off += align_up((size_t)p->width[l] * p->height[l], 64);
    }
    out->bytes = off;
    return DSDTM_OK;
}

static void pack_pyramid(const dsdtm_pyramid* p, const PackedPyr& pl, uint8_t* dst) {
    for (int l = 0; l < pl.levels; ++l) {
        copy_rows(dst + pl.off[l], (size_t)pl.w[l], p->data[l], (size_t)p->stride[l], (size_t)pl.w[l], (size_t)pl.h[l]);
    }
}

// the two pyramids of one alignment have the same geometry (the message says which level does not)
static int check_ref_cur_geometry(dsdtm_ctx* ctx, const PackedPyr& pr, const PackedPyr& pc) {
    if (pr.levels != pc.levels) { set_err(ctx, "ref/cur pyramids differ in level count"); return DSDTM_ERR_INVALID; }
    for (int l = 0; l < pr.levels; ++l)
        if (pr.w[l] != pc.w[l] || pr.h[l] != pc.h[l]) { set_err(ctx, "ref/cur level %d differ in size", l); return DSDTM_ERR_INVALID; }
    return DSDTM_OK;
}

// One alignment on the context's stream. The pyramids are either packed into the staging buffer
// together with the features (ref/cur given, dev_ref/dev_cur null) or already on the device.
static int sparse_align_one(dsdtm_ctx* ctx, const PackedPyr& pl, const dsdtm_pyramid* ref, const dsdtm_pyramid* cur,
                            const uint8_t* dev_ref, const uint8_t* dev_cur, size_t dev_pitch,
                            const dsdtm_camera* cam, const float* px_xy, const double* bearing,
                            const double* p_world, const uint8_t* initial, int n_features,
                            const double T_ref_w[12], double T_cur_w[12], const dsdtm_align_params* prm,
                            int* n_tracked, dsdtm_align_stats* stats, unsigned long long frames_seq = 0) {
    if (int rc = validate_params(ctx, prm, pl.levels)) return rc;
    if (int rc = frames_consume(ctx, frames_seq, ctx->stream)) return rc;
    // Run() (:34-38): too few features -> 0, pose untouched. Decided on the host: no launch needed.
    if (stats) memset(stats, 0, sizeof *stats);
    *n_tracked = 0;
    if (n_features < prm->min_fts || prm->max_level - 1 < prm->min_level) return DSDTM_OK;

    const bool staged_pyr = dev_ref == nullptr;
    const size_t nf = (size_t)n_features;
    const size_t pitch = staged_pyr ? align_up(pl.bytes, 256) : dev_pitch;
    // (its own column order: what goes up first, then the seed, which is read and written, then what only comes back; the poses
    // and the count take a 256-byte cell each)
    StageLayout lay;
    const size_t o_ref = lay.take(staged_pyr ? pitch : 0), o_cur = lay.take(staged_pyr ? pitch : 0), o_bear = lay.take(nf * 24),
                 o_pw = lay.take(nf * 24), o_tr = lay.take(256), o_px = lay.take(nf * 8), o_ini = lay.take(nf);
    const size_t in_bytes = lay.off;
    const size_t o_tc = lay.take(256),        // in (seed) and out
                 o_nt = lay.take(256), o_st = lay.take(sizeof(dsdtm_align_stats));
    const size_t total = lay.off;
    if (int rc = ensure_stage(ctx, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    if (staged_pyr) {
        pack_pyramid(ref, pl, h + o_ref);
        pack_pyramid(cur, pl, h + o_cur);
    }
    memcpy(h + o_bear, bearing, nf * 24);
    memcpy(h + o_pw, p_world, nf * 24);
    memcpy(h + o_tr, T_ref_w, 96);
    memcpy(h + o_px, px_xy, nf * 8);
    memcpy(h + o_ini, initial, nf);
    memcpy(h + o_tc, T_cur_w, 96);
    // Resident frames: the kernel reads features and poses straight from the pinned staging block (once per
    // pair, ~17 KB over PCIe) and writes its few results there: no H2D / D2H copy operations around the launch.
    const bool zero_copy = !staged_pyr;
    if (zero_copy) {
        if (int rc = pinned_device_ptr(ctx, &d)) return rc;
        memset(h + o_nt, 0, total - o_nt);
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(d, h, in_bytes + 256, hipMemcpyHostToDevice, ctx->stream));
    }

    dsdtm_batch_desc b;
    memset(&b, 0, sizeof b);
    b.n_pairs = 1; b.max_features = n_features; b.pyr_pitch = pitch;
    fill_levels(b, pl);
    b.ref_pyr = staged_pyr ? d + o_ref : dev_ref; b.cur_pyr = staged_pyr ? d + o_cur : dev_cur;
    b.px_xy = (const float*)(d + o_px);
    b.bearing = (const double*)(d + o_bear); b.p_world = (const double*)(d + o_pw); b.initial = d + o_ini;
    b.n_features = nullptr; b.T_ref_w = (const double*)(d + o_tr); b.T_cur_w = (double*)(d + o_tc);
    b.n_tracked = (int32_t*)(d + o_nt); b.stats = (dsdtm_align_stats*)(d + o_st);
    // Synchronous single-pair entry: its own timeout word, settled right here. A team launch whose wait for a partner
    // workgroup ran out (a foreign load on the device) is re-run on the one-CU kernels from the seed pose, which is
    // still in the pinned block: Run never fails for scheduling reasons (src/Sprase_ImageAlign.cpp:29-60).
    volatile unsigned* h_flag = ctx->h_flags + dsdtm_ctx::FLAG_SINGLE;
    *h_flag = 0;
    LaunchMode mode;
    mode.single = true;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool multi_cu = false;
        if (int rc_launch = launch_batch(ctx, &b, cam, prm, ctx->stream, mode, &multi_cu)) return rc_launch;
        if (!zero_copy) HIP_TRY(ctx, hipMemcpyAsync(h + o_tc, d + o_tc, total - o_tc, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        frames_settle(ctx);
        if (!*h_flag) break;
        *h_flag = 0;
        if (!multi_cu || attempt == 1 || options().no_recover) {
            clear_stream_counters(ctx, ctx->stream);
            set_err(ctx, multi_cu ? "sparse-align kernel: a wait for a partner workgroup timed out (re-run disabled: no_recover)"
                                  : "sparse-align kernel: intra-workgroup hand-over timed out");
            return DSDTM_ERR_HIP;
        }
        memcpy(h + o_tc, T_cur_w, 96);                      // the seed again
        if (zero_copy) memset(h + o_nt, 0, total - o_nt);
        else HIP_TRY(ctx, hipMemcpyAsync(d + o_tc, h + o_tc, 96, hipMemcpyHostToDevice, ctx->stream));
        mode.one_cu = true;
        ctx->recovered += 1;
    }
    memcpy(T_cur_w, h + o_tc, 96);
    *n_tracked = *(const int32_t*)(h + o_nt);
    if (stats) memcpy(stats, h + o_st, sizeof *stats);
    return DSDTM_OK;
}

extern "C" int dsdtm_sparse_align(dsdtm_ctx* ctx, const dsdtm_pyramid* ref, const dsdtm_pyramid* cur,
                                  const dsdtm_camera* cam, const float* px_xy, const double* bearing,
                                  const double* p_world, const uint8_t* initial, int n_features,
                                  const double T_ref_w[12], double T_cur_w[12], const dsdtm_align_params* prm,
                                  int* n_tracked, dsdtm_align_stats* stats) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!ref || !cur || !cam || !T_ref_w || !T_cur_w || !n_tracked || n_features < 0 ||
        (n_features > 0 && (!px_xy || !bearing || !p_world || !initial))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    PackedPyr pr, pc;
    if (int rc = plan_pyramid(ctx, ref, &pr)) return rc;
    if (int rc = plan_pyramid(ctx, cur, &pc)) return rc;
    if (int rc = check_ref_cur_geometry(ctx, pr, pc)) return rc;
    return sparse_align_one(ctx, pr, ref, cur, nullptr, nullptr, 0, cam, px_xy, bearing, p_world, initial, n_features,
                            T_ref_w, T_cur_w, prm, n_tracked, stats);
}

// ---- frames that stay on the device --------------------------------------------------------------
// The frame pool is shared with dsdtm_frame_destroy, which may run on any thread (a garbage collector's): it is touched only
// under g_live_mutex, held across the liveness check of the context — dsdtm_destroy takes a context off the live list under
// the same lock before it frees the pool.
uint8_t* dsdtm::detail::pool_take(dsdtm_ctx* ctx, size_t bytes, unsigned long long* seq) {
    std::lock_guard<std::mutex> g(g_live_mutex);
    for (size_t i = 0; i < ctx->frame_pool.size(); ++i)
        if (ctx->frame_pool[i].pitch == bytes) {                // a destroyed frame's buffer of this size (its users have drained:
            uint8_t* d = ctx->frame_pool[i].d;                  // every entry that takes a dsdtm_frame waits for its stream)
            *seq = ctx->frame_pool[i].seq;                      // (its prefetch may not have: the next user waits for that)
            ctx->frame_pool.erase(ctx->frame_pool.begin() + (long)i);
            return d;
        }
    return nullptr;
}

// its own, LIVE context on the same device: the buffer goes to that context's pool (no hipFree, which would wait for the whole
// device); false: the caller frees it
bool dsdtm::detail::pool_give(dsdtm_ctx* ctx, dsdtm_ctx* owner, int device, uint8_t* d, size_t bytes, unsigned long long seq) {
    if (!ctx || !d || owner != ctx) return false;
    std::lock_guard<std::mutex> g(g_live_mutex);
    if (!ctx_is_live_locked(ctx) || ctx->device != device || ctx->frame_pool.size() >= dsdtm_ctx::FRAME_POOL) return false;
    try { ctx->frame_pool.push_back(dsdtm_ctx::PooledFrame{bytes, d, seq}); } catch (...) { return false; }
    return true;
}

// `stream`: the stream that will write the new frame. with_depth: room for the float depth plane behind the pyramid.
int dsdtm::detail::frame_alloc(dsdtm_ctx* ctx, const PackedPyr& pl, hipStream_t stream, dsdtm_frame** out, bool with_depth) {
    dsdtm_frame* f = new (std::nothrow) dsdtm_frame();
    if (!f) return DSDTM_ERR_NOMEM;
    f->owner = ctx; f->device = ctx->device; f->pl = pl; f->pitch = align_up(pl.bytes, 256);
    f->bytes = f->pitch + (with_depth ? align_up((size_t)pl.w[0] * pl.h[0] * sizeof(float), 256) : 0);
    unsigned long long pooled_seq = 0;
    f->d = pool_take(ctx, f->bytes, &pooled_seq);
    if (f->d) {
        // the buffer of a frame that was destroyed while its prefetch was pending: that prefetch still writes it
        if (int rc = frames_consume(ctx, pooled_seq, stream)) {
            if (!pool_give(ctx, ctx, ctx->device, f->d, f->bytes, pooled_seq)) (void)hipFree(f->d);
            delete f;
            return rc;
        }
    } else if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void**)&f->d, f->bytes) != hipSuccess) {
        set_err(ctx, "hipMalloc of a %zu-byte frame failed", f->bytes);
        delete f;
        return DSDTM_ERR_NOMEM;
    }
    if (with_depth) f->depth = (float*)(f->d + f->pitch);
    *out = f;
    return DSDTM_OK;
}

extern "C" int dsdtm_frame_create(dsdtm_ctx* ctx, const dsdtm_pyramid* pyr, dsdtm_frame** out) {
    if (!ctx || !out) return DSDTM_ERR_INVALID;
    *out = nullptr;
    PackedPyr pl;
    if (int rc = plan_pyramid(ctx, pyr, &pl)) return rc;
    if (int rc = ensure_stage(ctx, pl.bytes)) return rc;
    dsdtm_frame* f = nullptr;
    if (int rc = frame_alloc(ctx, pl, ctx->stream, &f)) return rc;
    pack_pyramid(pyr, pl, (uint8_t*)ctx->h_pinned);
    hipError_t e = hipMemcpyAsync(f->d, ctx->h_pinned, pl.bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the pinned buffer is reused by the next call
    if (e != hipSuccess) { set_err(ctx, "frame upload failed: %s", hipGetErrorString(e)); dsdtm_frame_destroy(ctx, f); return DSDTM_ERR_HIP; }
    frames_settle(ctx);
    *out = f;
    return DSDTM_OK;
}

extern "C" int dsdtm_frame_create_from_image(dsdtm_ctx* ctx, const uint8_t* level0, int width, int height, int stride,
                                             int levels, dsdtm_frame** out) {
    if (!ctx || !out) return DSDTM_ERR_INVALID;
    *out = nullptr;
    if (!level0 || width <= 0 || height <= 0 || stride < width || levels <= 0 || levels > DSDTM_MAX_LEVELS) {
        set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID;
    }
    PackedPyr pl;
    int st[DSDTM_MAX_LEVELS];
    plan_image_pyramid(width, height, levels, &pl, st);
    if (int rc = ensure_stage(ctx, (size_t)width * height)) return rc;
    dsdtm_frame* f = nullptr;
    if (int rc = frame_alloc(ctx, pl, ctx->stream, &f)) return rc;
    uint8_t* hp = (uint8_t*)ctx->h_pinned;
    copy_rows(hp, (size_t)width, level0, (size_t)stride, (size_t)width, (size_t)height);
    // level 0 enters through a kernel on the compute stream (ingest_kernel, pyrdown.hip): no copy operation in front of the
    // pyramid kernel — the hand-over from the copy engine to the compute queue costs more than the 8 us of the copy itself
    void* hpd = nullptr;
    hipError_t e = hipHostGetDevicePointer(&hpd, hp, 0);
    if (e == hipSuccess) e = ingest_launch(hpd, f->d, (size_t)width * height, nullptr, nullptr, 0, ctx->stream);
    int rc = DSDTM_OK;
    if (e == hipSuccess) rc = dsdtm_pyrdown_batch_device(ctx, f->d, f->pitch, 1, levels, pl.w, pl.h, st, pl.off, ctx->stream);
    if (e == hipSuccess && rc == DSDTM_OK) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || rc != DSDTM_OK) {
        if (e != hipSuccess) { set_err(ctx, "frame upload failed: %s", hipGetErrorString(e)); rc = DSDTM_ERR_HIP; }
        dsdtm_frame_destroy(ctx, f);
        return rc;
    }
    frames_settle(ctx);
    *out = f;
    return DSDTM_OK;
}

extern "C" void dsdtm_frame_destroy(dsdtm_ctx* ctx, dsdtm_frame* f) {
    if (!f) return;
    if (FrameSlab* sl = f->slab) {                                   // a frame of a batch: the slab goes with its last frame
        delete f;
        if (sl->refs.fetch_sub(1) != 1) return;
        if (!pool_give(ctx, sl->owner, sl->device, sl->d, sl->bytes)) { (void)hipSetDevice(sl->device); if (sl->d) (void)hipFree(sl->d); }
        delete sl;
        return;
    }
    // (a frame whose prefetch is still pending: the buffer goes to the pool with the frame's number, and its next user's
    // stream waits for the event behind it — frame_alloc)
    if (pool_give(ctx, f->owner, f->device, f->d, f->bytes, f->seq)) { delete f; return; }
    (void)hipSetDevice(f->device);
    if (f->d) (void)hipFree(f->d);       // hipFree waits for the device's pending work
    delete f;
}

// ---- RGB-D frames that enter the device ahead of time --------------------------------------------------------------
// rgbd.hip defines these; weak here so that a host-only build of this file without the kernels (the fake-HIP sanitizer
// drivers under tests/ that do not fake them) still links. The entry points test them and fail cleanly where they are missing.
namespace dsdtm {
__attribute__((weak)) hipError_t depth_ingest_launch(const uint16_t* src, int src_stride, float* dst, int w, int h, float inv_scale,
                                                     int num_cus, hipStream_t stream);
__attribute__((weak)) hipError_t lift_launch(const LiftArgs& args, hipStream_t stream);
}

// Where an image of the caller lives (0: ordinary host memory, 1: pinned host memory, 2: this device's memory; -1: another device's, *device)
static int image_memory(dsdtm_ctx* ctx, const void* p, int* device = nullptr) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return 0; }    // (an ordinary host pointer: not an error)
    if (device) *device = pa_.device;
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? 2 : -1;
    return pa_.type == hipMemoryTypeHost ? 1 : 0;
}

// clear_unaligned: the HIP error state is cleared for an odd-address pinned image too, although nothing failed (dsdtm_track_frames
// and dsdtm_frame_prefetch do, dsdtm_track_frame does not: kept as each was). known_mem: image_memory(ptr), where the caller has it.
ImageRoute dsdtm::detail::route_image(dsdtm_ctx* ctx, const void* ptr, int width, int stride, bool clear_unaligned, const int* known_mem) {
    ImageRoute r = {STAGED, nullptr, 0};
    const int mem = known_mem ? *known_mem : image_memory(ctx, ptr, &r.device);
    const bool contiguous = stride == width, aligned = !(((size_t)ptr) & 15);
    if (mem < 0) r.route = OTHER_DEVICE;
    else if (mem == 2) { r.route = contiguous && aligned ? IN_PLACE : COPY_D2D; r.dev = contiguous && aligned ? ptr : nullptr; }
    else if (mem == 1 && contiguous) {
        void* p_ = nullptr;
        r.route = COPY_H2D;
        if (aligned && hipHostGetDevicePointer(&p_, (void*)ptr, 0) == hipSuccess) { r.route = IN_PLACE; r.dev = p_; }
        else if (aligned || clear_unaligned) (void)hipGetLastError();
    }
    return r;
}
// Level 0 of `image` into dst (dense rows) by its route. run (may be NULL): moved by the same ingest launch; behind a copy-engine
// route it gets an ingest launch of its own, with no image.
int dsdtm::detail::enqueue_level0(dsdtm_ctx* ctx, const ImageRoute& r, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                                  const RunRange* run, hipStream_t stream) {
    const size_t W = (size_t)width, H = (size_t)height;
    if (r.route == COPY_D2D || r.route == COPY_H2D) {
        if (r.route == COPY_D2D) HIP_TRY(ctx, hipMemcpy2DAsync(dst, W, image, (size_t)stride, W, H, hipMemcpyDeviceToDevice, stream));
        else HIP_TRY(ctx, hipMemcpyAsync(dst, image, W * H, hipMemcpyHostToDevice, stream));
        if (run) HIP_TRY(ctx, ingest_launch(nullptr, nullptr, 0, run->src, run->dst, run->bytes, stream));
        return DSDTM_OK;
    }
    HIP_TRY(ctx, ingest_launch(r.dev, dst, W * H, run ? run->src : nullptr, run ? run->dst : nullptr, run ? run->bytes : 0, stream));
    return DSDTM_OK;
}

// Frame construction (src/Frame.cpp:35-41) off the tracked frame's chain: level 0, the pyramid and the depth conversion are
// enqueued on the context's prefetch stream, an event is recorded behind them and the call returns.
extern "C" int dsdtm_frame_prefetch(dsdtm_ctx* ctx, const dsdtm_frame_image* im, dsdtm_frame** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "prefetch: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    if (!im) { set_err(ctx, "prefetch: image is NULL"); return DSDTM_ERR_INVALID; }
    if (!im->gray) { set_err(ctx, "prefetch: image->gray is NULL"); return DSDTM_ERR_INVALID; }
    if (im->width <= 0 || im->height <= 0 || im->stride < im->width || im->levels <= 0 || im->levels > DSDTM_MAX_LEVELS ||
        im->width > 16384 || im->height > 16384) {
        set_err(ctx, "prefetch: bad image geometry (width %d, height %d, stride %d, levels %d)", im->width, im->height, im->stride, im->levels);
        return DSDTM_ERR_INVALID;
    }
    if (im->depth && (im->depth_stride < im->width || !(im->depth_scale > 0.0f))) {
        set_err(ctx, "prefetch: bad depth map (depth_stride %d < width %d, or depth_scale %g not positive)", im->depth_stride, im->width, (double)im->depth_scale);
        return DSDTM_ERR_INVALID;
    }
    if (im->depth && !depth_ingest_launch) { set_err(ctx, "prefetch: this build has no depth kernels"); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        // (the call allocates, waits for events and records one on a stream of its own: none of that can be part of a capture)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) { set_err(ctx, "prefetch: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    }
    const int gray_mem = image_memory(ctx, im->gray), depth_mem = im->depth ? image_memory(ctx, im->depth) : 0;   // (the depth map: its memory kind only — no alignment rule, no 2-D copy)
    if (gray_mem < 0 || depth_mem < 0) { set_err(ctx, "prefetch: image->%s lives on another device than the context's (%d)", gray_mem < 0 ? "gray" : "depth", ctx->device); return DSDTM_ERR_INVALID; }
    if (!ctx->prefetch_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->prefetch_stream, hipStreamNonBlocking));
    {
        hipEvent_t& e = ctx->prefetch_event[(ctx->prefetch_seq + 1) % dsdtm_ctx::PREFETCH_EVENTS];    // this frame's
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    hipStream_t ps = ctx->prefetch_stream;
    PackedPyr pl;
    int st[DSDTM_MAX_LEVELS];
    plan_image_pyramid(im->width, im->height, im->levels, &pl, st);
    const size_t W = (size_t)im->width, H = (size_t)im->height, img = W * H;
    // how each image travels (the gray image as in dsdtm_track_frame): read in place by a kernel, moved by the copy engine
    // from where it is, or staged — copied into a slot of the prefetch ring now, so that the caller's buffer is free on return
    ImageRoute gray = route_image(ctx, im->gray, im->width, im->stride, true, &gray_mem);
    const bool gray_staged = gray.route == STAGED;
    const uint16_t* depth_dev = nullptr;                     // the depth map as the kernel sees it
    int depth_dev_stride = im->depth_stride;
    bool depth_staged = false;
    if (im->depth) {
        if (depth_mem == 2) depth_dev = im->depth;
        else if (depth_mem == 1) {
            void* p_ = nullptr;
            if (hipHostGetDevicePointer(&p_, (void*)im->depth, 0) == hipSuccess) depth_dev = (const uint16_t*)p_;
            else { (void)hipGetLastError(); depth_staged = true; }
        } else depth_staged = true;
    }
    const size_t s_gray = 0, s_depth = gray_staged ? align_up(img, 256) : 0;
    const size_t stage_bytes = s_depth + (depth_staged ? img * sizeof(uint16_t) : 0);
    dsdtm_ctx::PrefetchSlot* slot = nullptr;
    if (stage_bytes) {
        slot = &ctx->prefetch_slot[ctx->prefetch_next_slot & 1u];
        // the frame that used this slot last may still be reading it
        if (slot->seq > ctx->prefetch_settled) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->prefetch_event[slot->seq % dsdtm_ctx::PREFETCH_EVENTS]));
            ctx->prefetch_settled = slot->seq;
        }
        if (stage_bytes > slot->cap) {
            if (slot->h) (void)hipHostFree(slot->h);
            slot->h = nullptr; slot->cap = 0;
            const size_t cap = align_up(stage_bytes + stage_bytes / 4, 1 << 16);
            HIP_TRY(ctx, hipHostMalloc(&slot->h, cap, hipHostMallocDefault));
            slot->cap = cap;
        }
    }
    dsdtm_frame* f = nullptr;
    if (int rc = frame_alloc(ctx, pl, ps, &f, im->depth != nullptr)) return rc;
    // on any failure: no frame, nothing pending (what was enqueued is waited for), the slot and the numbering untouched
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(ps);
        dsdtm_frame_destroy(ctx, f);
        return rc;
    };
    uint8_t* sh = slot ? (uint8_t*)slot->h : nullptr;
    uint8_t* shd = nullptr;                                  // the slot as the device sees it
    if (slot) { void* p_ = nullptr; API_TRY(hipHostGetDevicePointer(&p_, slot->h, 0)); shd = (uint8_t*)p_; }
    if (gray_staged) {
        copy_rows(sh + s_gray, W, im->gray, (size_t)im->stride, W, H);
        gray.dev = shd + s_gray;
    }
    if (depth_staged) {
        copy_rows(sh + s_depth, W * sizeof(uint16_t), im->depth, (size_t)im->depth_stride * sizeof(uint16_t), W * sizeof(uint16_t), H);
        depth_dev = (const uint16_t*)(shd + s_depth); depth_dev_stride = im->width;
    }
    // level 0 by a kernel where a kernel can read it (ingest_kernel, pyrdown.hip), else by the copy engine (a pinned image
    // at an odd address or one the device cannot address; a strided or odd device image), then the pyramid
    if (int rc = enqueue_level0(ctx, gray, im->gray, im->width, im->height, im->stride, f->d, nullptr, ps)) return fail(rc);
    if (int rc = dsdtm_pyrdown_batch_device(ctx, f->d, f->pitch, 1, pl.levels, pl.w, pl.h, st, pl.off, ps)) return fail(rc);
    if (im->depth) API_TRY(depth_ingest_launch(depth_dev, depth_dev_stride, f->depth, im->width, im->height, 1.0f / im->depth_scale, ctx->num_cus, ps));
    const unsigned long long seq = ctx->prefetch_seq + 1;
    API_TRY(hipEventRecord(ctx->prefetch_event[seq % dsdtm_ctx::PREFETCH_EVENTS], ps));
    ctx->prefetch_seq = seq;
    f->seq = seq;
    if (slot) { slot->seq = seq; ctx->prefetch_next_slot += 1; }
    *out = f;
    return DSDTM_OK;
}

extern "C" int dsdtm_frame_wait(dsdtm_ctx* ctx, const dsdtm_frame* f) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!f) { set_err(ctx, "frame_wait: frame is NULL"); return DSDTM_ERR_INVALID; }
    if (f->owner != ctx) { set_err(ctx, "frame belongs to another context"); return DSDTM_ERR_INVALID; }
    if (f->seq <= ctx->prefetch_settled) return DSDTM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->prefetch_event[f->seq % dsdtm_ctx::PREFETCH_EVENTS]));
    ctx->prefetch_settled = f->seq;
    return DSDTM_OK;
}

// Frame::Get_FeatureDetph(cv::Point2f) + Frame::UnProject (src/Frame.cpp:152-157, 201-224) for n pixels of a resident frame.
extern "C" int dsdtm_frame_lift(dsdtm_ctx* ctx, const dsdtm_frame* f, const dsdtm_camera* cam, const double* T_c2w,
                                const float* px_xy, int n, float* depth_out, double* p_world_out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!f) { set_err(ctx, "lift: frame is NULL"); return DSDTM_ERR_INVALID; }
    if (!cam) { set_err(ctx, "lift: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!T_c2w) { set_err(ctx, "lift: T_c2w is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_LIFT_MAX) { set_err(ctx, "lift: n = %d outside 0..%d", n, DSDTM_LIFT_MAX); return DSDTM_ERR_INVALID; }
    if (n > 0 && (!px_xy || !depth_out || !p_world_out)) {
        set_err(ctx, "lift: %s is NULL", !px_xy ? "px_xy" : !depth_out ? "depth_out" : "p_world_out"); return DSDTM_ERR_INVALID;
    }
    if (f->owner != ctx) { set_err(ctx, "frame belongs to another context"); return DSDTM_ERR_INVALID; }
    if (!f->depth) { set_err(ctx, "lift: the frame has no depth map (dsdtm_frame_image.depth was NULL)"); return DSDTM_ERR_INVALID; }
    if (!lift_launch) { set_err(ctx, "lift: this build has no depth kernels"); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    const size_t N = (size_t)n;
    StageLayout lay;
    const size_t o_px = lay.take(N * 8), o_d = lay.take(N * 4), o_p = lay.take(N * 24);
    if (int rc = ensure_stage(ctx, lay.off)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* hd = nullptr;
    if (int rc = pinned_device_ptr(ctx, &hd)) return rc;
    memcpy(h + o_px, px_xy, N * 8);
    // every input is read once and every result written once: straight from / to the pinned block
    LiftArgs a;
    memset(&a, 0, sizeof a);
    a.depth = f->depth; a.w = f->pl.w[0]; a.h = f->pl.h[0];
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    memcpy(a.T, T_c2w, 96);
    a.px_xy = (const float*)(hd + o_px); a.depth_out = (float*)(hd + o_d); a.p_world = (double*)(hd + o_p); a.n = n;
    if (int rc = frames_consume(ctx, f->seq, ctx->stream)) return rc;
    HIP_TRY(ctx, lift_launch(a, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    frames_settle(ctx);
    memcpy(depth_out, h + o_d, N * 4);
    memcpy(p_world_out, h + o_p, N * 24);
    return DSDTM_OK;
}

extern "C" int dsdtm_sparse_align_frames(dsdtm_ctx* ctx, const dsdtm_frame* ref, const dsdtm_frame* cur,
                                         const dsdtm_camera* cam, const float* px_xy, const double* bearing,
                                         const double* p_world, const uint8_t* initial, int n_features,
                                         const double T_ref_w[12], double T_cur_w[12], const dsdtm_align_params* prm,
                                         int* n_tracked, dsdtm_align_stats* stats) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!ref || !cur || !cam || !T_ref_w || !T_cur_w || !n_tracked || n_features < 0 ||
        (n_features > 0 && (!px_xy || !bearing || !p_world || !initial))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    if (ref->owner != ctx || cur->owner != ctx) { set_err(ctx, "frame belongs to another context"); return DSDTM_ERR_INVALID; }
    if (int rc = check_ref_cur_geometry(ctx, ref->pl, cur->pl)) return rc;
    return sparse_align_one(ctx, ref->pl, nullptr, nullptr, ref->d, cur->d, ref->pitch, cam, px_xy, bearing, p_world, initial,
                            n_features, T_ref_w, T_cur_w, prm, n_tracked, stats, ref->seq > cur->seq ? ref->seq : cur->seq);
}

// ---- feature detector (per-cell part) ----------------------------------------------------------
// levels: of the pyramid the detector is to run on
static int check_detect_params(dsdtm_ctx* ctx, const dsdtm_detect_params* prm, int levels) {
    if (prm->cell_size <= 0 || prm->grid_cols <= 0 || prm->grid_rows <= 0 || prm->levels <= 0 || prm->levels > levels ||
        prm->barrier < 0 || prm->barrier > 254 || !(prm->detection_threshold >= 0.0f) ||
        (long long)prm->grid_cols * prm->grid_rows > (1 << 24)) {
        set_err(ctx, "bad detector parameters"); return DSDTM_ERR_INVALID;
    }
    return DSDTM_OK;
}
// what both detector entries pass on from the parameters
static void fill_detect_params(DetectArgs& a, const dsdtm_detect_params* prm, size_t pyr_pitch, int n_frames) {
    a.pyr_pitch = pyr_pitch; a.n_frames = n_frames; a.levels = prm->levels;
    a.cell_size = prm->cell_size; a.grid_cols = prm->grid_cols; a.grid_rows = prm->grid_rows; a.barrier = prm->barrier;
    a.detection_threshold = prm->detection_threshold;
}
static int detect_cells_one(dsdtm_ctx* ctx, const PackedPyr& pl, const dsdtm_pyramid* host_pyr, const uint8_t* dev_pyr,
                            const uint8_t* grid_occupied, const dsdtm_detect_params* prm, float* cell_score,
                            int32_t* cell_x, int32_t* cell_y, int32_t* cell_level, unsigned long long frame_seq = 0) {
    if (!prm || !cell_score || !cell_x || !cell_y || !cell_level) { set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID; }
    if (int rc = check_detect_params(ctx, prm, pl.levels)) return rc;
    for (int l = 0; l < prm->levels; ++l)
        if (pl.w[l] >= (1 << 14) || pl.h[l] >= (1 << 14)) { set_err(ctx, "level %d larger than 16383 pixels", l); return DSDTM_ERR_INVALID; }
    const size_t G = (size_t)prm->grid_cols * prm->grid_rows;
    const size_t pitch = align_up(pl.bytes, 256);
    StageLayout lay;
    const size_t o_pyr = lay.take(dev_pyr ? 0 : pitch), o_occ = lay.take(G);
    const size_t in_bytes = lay.off;
    const size_t o_key = lay.take(G * 8), o_score = lay.take(pitch);
    if (int rc = ensure_stage(ctx, lay.off)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    if (!dev_pyr) pack_pyramid(host_pyr, pl, h + o_pyr);
    if (grid_occupied) memcpy(h + o_occ, grid_occupied, G); else memset(h + o_occ, 0, G);
    if (int rc = frames_consume(ctx, frame_seq, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d + o_key, 0, G * 8, ctx->stream));
    DetectArgs a;
    memset(&a, 0, sizeof a);
    a.pyr = dev_pyr ? dev_pyr : d + o_pyr; a.score = d + o_score; a.cell_key = (unsigned long long*)(d + o_key);
    a.occupied = d + o_occ;
    fill_detect_params(a, prm, pitch, 1);
    fill_levels(a.lv, pl, prm->levels);
    HIP_TRY(ctx, detect_launch(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + o_key, d + o_key, G * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    frames_settle(ctx);
    const unsigned long long* keys = (const unsigned long long*)(h + o_key);
    for (size_t k = 0; k < G; ++k) {
        if (!keys[k]) { cell_score[k] = prm->detection_threshold; cell_x[k] = 0; cell_y[k] = 0; cell_level[k] = 0; continue; }   // :74
        const uint32_t bits = (uint32_t)(keys[k] >> 32), order = 0xffffffffu - (uint32_t)keys[k];
        const int L = (int)(order >> 28), y = (int)((order >> 14) & 0x3fffu), x = (int)(order & 0x3fffu);
        memcpy(&cell_score[k], &bits, 4);
        cell_x[k] = x << L; cell_y[k] = y << L; cell_level[k] = L;                                  // :106
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_detect_cells(dsdtm_ctx* ctx, const dsdtm_pyramid* pyr, const uint8_t* grid_occupied,
                                  const dsdtm_detect_params* prm, float* cell_score, int32_t* cell_x, int32_t* cell_y,
                                  int32_t* cell_level) {
    if (!ctx) return DSDTM_ERR_INVALID;
    PackedPyr pl;
    if (int rc = plan_pyramid(ctx, pyr, &pl)) return rc;
    return detect_cells_one(ctx, pl, pyr, nullptr, grid_occupied, prm, cell_score, cell_x, cell_y, cell_level);
}

extern "C" int dsdtm_detect_cells_frame(dsdtm_ctx* ctx, const dsdtm_frame* frame, const uint8_t* grid_occupied,
                                        const dsdtm_detect_params* prm, float* cell_score, int32_t* cell_x, int32_t* cell_y,
                                        int32_t* cell_level) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!frame) { set_err(ctx, "NULL frame"); return DSDTM_ERR_INVALID; }
    if (frame->owner != ctx) { set_err(ctx, "frame belongs to another context"); return DSDTM_ERR_INVALID; }
    return detect_cells_one(ctx, frame->pl, nullptr, frame->d, grid_occupied, prm, cell_score, cell_x, cell_y, cell_level, frame->seq);
}

// The image part of Feature_detector::detect for n_frames packed device pyramids in one go (independent sequences,
// keyframes of an offline run): every pointer is a device pointer, nothing is copied, asynchronous on hip_stream.
extern "C" int dsdtm_detect_cells_batch_device(dsdtm_ctx* ctx, const uint8_t* pyr, size_t pyr_pitch, int n_frames, int levels,
                                               const int* width, const int* height, const int* stride, const size_t* level_offset,
                                               const uint8_t* grid_occupied, const dsdtm_detect_params* prm,
                                               uint8_t* score_scratch, unsigned long long* key_scratch,
                                               float* cell_score, int32_t* cell_x, int32_t* cell_y, int32_t* cell_level,
                                               void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!pyr || !width || !height || !stride || !level_offset || !prm || !score_scratch || !key_scratch || !cell_score || !cell_x ||
        !cell_y || !cell_level || n_frames < 0 || levels <= 0 || levels > DSDTM_MAX_LEVELS) { set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID; }
    if (int rc = check_detect_params(ctx, prm, levels)) return rc;
    // the kernels fetch pyramid and score rows as dwords and index frames through the grid's z dimension
    if ((pyr_pitch & 3) || (((size_t)pyr) & 3) || (((size_t)score_scratch) & 3)) {
        set_err(ctx, "detector batch: pyramid base, score scratch and pyr_pitch must be 4-byte aligned"); return DSDTM_ERR_INVALID;
    }
    if ((long long)n_frames * prm->levels > 65535) {
        set_err(ctx, "detector batch: n_frames * levels = %lld exceeds 65535 (one launch indexes frames through grid.z): split the batch",
                (long long)n_frames * prm->levels);
        return DSDTM_ERR_INVALID;
    }
    if (n_frames == 0) return DSDTM_OK;
    DetectArgs a;
    memset(&a, 0, sizeof a);
    for (int l = 0; l < prm->levels; ++l)       // (level by level with the size limit of the cell keys: the first bad level is the one named)
        if (width[l] >= (1 << 14) || height[l] >= (1 << 14) || !level_fits(l, width, height, stride, level_offset, pyr_pitch, a.lv)) {
            set_err(ctx, "level %d does not fit", l); return DSDTM_ERR_INVALID;
        }
    const size_t G = (size_t)prm->grid_cols * prm->grid_rows;
    a.pyr = pyr; a.score = score_scratch; a.cell_key = key_scratch; a.occupied = grid_occupied;
    a.cell_score = cell_score; a.cell_x = cell_x; a.cell_y = cell_y; a.cell_level = cell_level;
    fill_detect_params(a, prm, pyr_pitch, n_frames);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(key_scratch, 0, (size_t)n_frames * G * 8, (hipStream_t)hip_stream));
    HIP_TRY(ctx, detect_launch(a, (hipStream_t)hip_stream));
    return DSDTM_OK;
}

#ifdef DSDTM_DIAG
// Diagnostic (tests): the FAST-10 score map and the non-max survivors of ONE 8-bit image, as the detector's
// two passes produce them on the device. score/keep: width*height bytes each.
extern "C" int dsdtm_debug_fast10(dsdtm_ctx* ctx, const uint8_t* img, int width, int height, int stride, int barrier,
                                  uint8_t* score, uint8_t* keep) {
    if (!ctx || !img || !score || !keep || width <= 0 || height <= 0 || stride < width || width >= (1 << 14) || height >= (1 << 14))
        return DSDTM_ERR_INVALID;
    const size_t n = (size_t)width * height, pitch = align_up(n, 256);
    if (int rc = ensure_stage(ctx, 3 * pitch + 256)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    for (int y = 0; y < height; ++y) memcpy(h + (size_t)y * width, img + (size_t)y * stride, width);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d + pitch, 0, 2 * pitch + 256, ctx->stream));
    DetectArgs a;
    memset(&a, 0, sizeof a);
    a.pyr = d; a.score = d + pitch; a.keep = d + 2 * pitch; a.cell_key = (unsigned long long*)(d + 3 * pitch);
    a.cell_size = 1 << 20; a.grid_cols = 1; a.grid_rows = 1; a.barrier = barrier; a.detection_threshold = 3.0e38f;
    a.lv[0].w = width; a.lv[0].h = height; a.lv[0].stride = width; a.lv[0].off = 0;
    a.pyr_pitch = pitch; a.n_frames = 1; a.levels = 1;
    HIP_TRY(ctx, detect_launch(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h, d + pitch, 2 * pitch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(score, h, n);
    memcpy(keep, h + pitch, n);
    return DSDTM_OK;
}
#endif  // DSDTM_DIAG

// ---- Align2D ------------------------------------------------------------------------------
extern "C" int dsdtm_align2d_batch_device(dsdtm_ctx* ctx, const dsdtm_image_desc* cur, const uint8_t* patch_border,
                                          const uint8_t* patch, const int32_t* level, double* px_xy,
                                          uint8_t* converged, int max_iters, int m, void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cur || m < 0 || cur->levels <= 0 || cur->levels > DSDTM_MAX_LEVELS) { set_err(ctx, "bad image descriptor"); return DSDTM_ERR_INVALID; }
    if (m == 0) return DSDTM_OK;
    if (!cur->data || !patch_border || !patch || !level || !px_xy || !converged) { set_err(ctx, "NULL device pointer"); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    A2DKernelArgs a;
    memset(&a, 0, sizeof a);
    if (int rc = check_levels(ctx, cur->levels, cur->width, cur->height, cur->stride, cur->level_offset, cur->bytes, "", "the packed pyramid", a.lv)) return rc;
    a.cur_pyr = cur->data; a.patch_border = patch_border; a.patch = patch; a.level = level;
    a.px_xy = px_xy; a.converged = converged; a.m = m; a.max_iters = max_iters; a.levels = cur->levels;
    HIP_TRY(ctx, align2d_launch(a, (hipStream_t)hip_stream));
    return DSDTM_OK;
}

extern "C" int dsdtm_align2d_batch(dsdtm_ctx* ctx, const dsdtm_pyramid* cur, const uint8_t* patch_border,
                                   const uint8_t* patch, const int32_t* level, double* px_xy, uint8_t* converged,
                                   int max_iters, int m) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (m < 0 || (m > 0 && (!patch_border || !patch || !level || !px_xy || !converged))) { set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID; }
    PackedPyr pc;
    if (int rc = plan_pyramid(ctx, cur, &pc)) return rc;
    if (m == 0) return DSDTM_OK;
    for (int i = 0; i < m; ++i)
        if (level[i] < 0 || level[i] >= pc.levels) { set_err(ctx, "level[%d]=%d outside the pyramid", i, level[i]); return DSDTM_ERR_INVALID; }
    const size_t M = (size_t)m;
    StageLayout lay;
    const size_t o_pyr = lay.take(pc.bytes), o_pb = lay.take(M * 100), o_p = lay.take(M * 64), o_lv = lay.take(M * 4), o_px = lay.take(M * 16);
    const size_t in_bytes = lay.off;
    const size_t o_cv = lay.take(M);
    const size_t total = lay.off;
    if (int rc = ensure_stage(ctx, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    pack_pyramid(cur, pc, h + o_pyr);
    memcpy(h + o_pb, patch_border, M * 100);
    memcpy(h + o_p, patch, M * 64);
    memcpy(h + o_lv, level, M * 4);
    memcpy(h + o_px, px_xy, M * 16);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    dsdtm_image_desc img;
    memset(&img, 0, sizeof img);
    fill_levels(img, pc);
    img.bytes = pc.bytes; img.data = d + o_pyr;
    if (int rc = dsdtm_align2d_batch_device(ctx, &img, d + o_pb, d + o_p, (const int32_t*)(d + o_lv),
                                            (double*)(d + o_px), d + o_cv, max_iters, m, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h + o_px, d + o_px, total - o_px, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(px_xy, h + o_px, M * 16);
    memcpy(converged, h + o_cv, M);
    return DSDTM_OK;
}

// ---- pyrDown ------------------------------------------------------------------------------
extern "C" int dsdtm_pyrdown_batch_device(dsdtm_ctx* ctx, uint8_t* pyr, size_t pyr_pitch, int n_images, int levels,
                                          const int* width, const int* height, const int* stride,
                                          const size_t* level_offset, void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!pyr || !width || !height || !stride || !level_offset || levels <= 0 || levels > DSDTM_MAX_LEVELS || n_images < 0) {
        set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID;
    }
    for (int l = 0; l < levels; ++l) {
        if (!level_fits(l, width, height, stride, level_offset, pyr_pitch, nullptr)) { set_err(ctx, "level %d does not fit", l); return DSDTM_ERR_INVALID; }
        if (l > 0 && (width[l] != (width[l - 1] + 1) / 2 || height[l] != (height[l - 1] + 1) / 2)) {
            set_err(ctx, "level %d is not ((w+1)/2,(h+1)/2) of level %d", l, l - 1); return DSDTM_ERR_INVALID;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // Few images (the live tracker's new frame): ONE launch builds every level, intermediate levels in LDS — the call is
    // bound by launch latency and dependent round trips, 0.0145 -> 0.0079 ms for a 640x480x4 pyramid. Large batches are
    // bound by HBM and run one launch per level (the fused kernel's LDS stages issue no loads: 2..30 % slower from 64
    // images on, `tools/pyr_ab.py`). option pyr_fused = 0 / 2: never / whenever the shape allows (A/B, tests);
    // pyr_band: rows of the coarsest level per workgroup.
    const int fused_mode = options().pyr_fused;
    if (fused_mode == 2 || (fused_mode == 1 && n_images <= 32)) {
        bool launched = false;
        HIP_TRY(ctx, pyrdown_fused_launch(pyr, pyr_pitch, n_images, levels, width, height, stride, level_offset,
                                          options().pyr_band, (hipStream_t)hip_stream, &launched));
        if (launched) return DSDTM_OK;
    }
    for (int l = 1; l < levels; ++l)
        HIP_TRY(ctx, pyrdown_launch(pyr, pyr_pitch, n_images, width[l - 1], height[l - 1], stride[l - 1],
                                    level_offset[l - 1], stride[l], level_offset[l], (hipStream_t)hip_stream));
    return DSDTM_OK;
}

extern "C" int dsdtm_pyrdown(dsdtm_ctx* ctx, const uint8_t* level0, int width, int height, int stride, int levels,
                             uint8_t* const* out_levels, const int* out_stride) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!level0 || width <= 0 || height <= 0 || stride < width || levels <= 0 || levels > DSDTM_MAX_LEVELS ||
        (levels > 1 && (!out_levels || !out_stride))) { set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID; }
    PackedPyr pl;
    int st[DSDTM_MAX_LEVELS];
    plan_image_pyramid(width, height, levels, &pl, st);
    const int *w = pl.w, *h = pl.h;
    const size_t *off = pl.off, pitch = align_up(pl.bytes, 256);
    if (int rc = ensure_stage(ctx, pitch)) return rc;
    uint8_t* hp = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    copy_rows(hp, (size_t)width, level0, (size_t)stride, (size_t)width, (size_t)height);
    HIP_TRY(ctx, hipMemcpyAsync(d, hp, (size_t)width * height, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = dsdtm_pyrdown_batch_device(ctx, d, pitch, 1, levels, w, h, st, off, ctx->stream)) return rc;
    if (levels > 1) HIP_TRY(ctx, hipMemcpyAsync(hp + off[1], d + off[1], pl.bytes - off[1], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int l = 1; l < levels; ++l) {
        if (!out_levels[l] || out_stride[l] < w[l]) { set_err(ctx, "bad output level %d", l); return DSDTM_ERR_INVALID; }
        copy_rows(out_levels[l], (size_t)out_stride[l], hp + off[l], (size_t)w[l], (size_t)w[l], (size_t)h[l]);
    }
    return DSDTM_OK;
}

// ---- warp prelude ---------------------------------------------------------------------------
// The columns of FindMatchDirect's two kernels over m candidates, wherever an entry keeps them
struct MatchColumns {
    const double* T_kf_w; const int32_t* cand_kf; const float* ref_px; const int32_t* ref_level; const double* ref_bearing; const double* p_world;
    double* affine; int32_t* search_level; uint8_t* patch_border; uint8_t* patch;      // written by the warp half ...
    double* px_xy; uint8_t* converged;                                                  // ... and by Align2D (level-0 pixels)
};
// The arguments of the warp prelude on one level table: camera, columns, sizes. The caller adds where the pyramids lie (and, for
// a batch of current frames, their poses and the candidates' frames).
static void fill_warp_args(WarpKernelArgs& a, const MatchColumns& c, const dsdtm_camera* cam, const LevelGeom* lv, int levels, int m, int n_kf,
                           int max_search_level) {
    memset(&a, 0, sizeof a);
    a.T_kf_w = c.T_kf_w; a.cand_kf = c.cand_kf; a.ref_px = c.ref_px; a.ref_level = c.ref_level; a.ref_bearing = c.ref_bearing;
    a.p_world = c.p_world; a.affine = c.affine; a.search_level = c.search_level; a.patch_border = c.patch_border; a.patch = c.patch;
    a.m = m; a.n_kf = n_kf; a.max_search_level = max_search_level; a.levels = levels;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    for (int l = 0; l < levels; ++l) a.lv[l] = lv[l];
}
// ... and of the Align2D that follows it (b), on the prelude's patches and search levels
static void fill_match_args(WarpKernelArgs& a, A2DKernelArgs& b, const MatchColumns& c, const dsdtm_camera* cam, const LevelGeom* lv, int levels,
                            int m, int n_kf, int max_search_level, int max_iters) {
    fill_warp_args(a, c, cam, lv, levels, m, n_kf, max_search_level);
    memset(&b, 0, sizeof b);
    b.patch_border = c.patch_border; b.patch = c.patch; b.level = c.search_level; b.px_xy = c.px_xy; b.converged = c.converged;
    b.m = m; b.max_iters = max_iters; b.levels = levels; b.px_level0 = 1;
    for (int l = 0; l < levels; ++l) b.lv[l] = lv[l];
}
// FindMatchDirect as one kernel, the warped patches in LDS (a.patch_border / a.patch are not touched); the diagnostic build can
// split it into its two halves (option fmd_split, rounds 1-4), the patches then go through device memory
static int launch_match(dsdtm_ctx* ctx, WarpKernelArgs& a, const A2DKernelArgs& b, hipStream_t stream) {
#ifdef DSDTM_DIAG
    if (options().fmd_split) {
        HIP_TRY(ctx, warp_launch(a, stream));
        HIP_TRY(ctx, align2d_launch(b, stream));
        return DSDTM_OK;
    }
#endif
    a.affine = nullptr; a.no_xcd = options().fmd_no_xcd;                        // (nobody reads the affine maps here)
    HIP_TRY(ctx, match_launch(a, b, stream));
    return DSDTM_OK;
}
extern "C" int dsdtm_warp_patches(dsdtm_ctx* ctx, const dsdtm_pyramid* kf_pyr, int n_kf, const dsdtm_camera* cam,
                                  const double* T_kf_w, const double T_cur_w[12], const int32_t* cand_kf,
                                  const float* ref_px, const int32_t* ref_level, const double* ref_bearing,
                                  const double* p_world, int max_search_level, int m, double* affine,
                                  int32_t* search_level, uint8_t* patch_border, uint8_t* patch) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!kf_pyr || n_kf <= 0 || !cam || !T_kf_w || !T_cur_w || m < 0 ||
        (m > 0 && (!cand_kf || !ref_px || !ref_level || !ref_bearing || !p_world || !search_level || !patch_border || !patch))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    if (m == 0) return DSDTM_OK;
    PackedPyr p0;
    if (int rc = plan_pyramid(ctx, &kf_pyr[0], &p0)) return rc;
    for (int k = 1; k < n_kf; ++k) {
        PackedPyr pk;
        if (int rc = plan_pyramid(ctx, &kf_pyr[k], &pk)) return rc;
        if (!same_geometry(pk, p0)) { set_err(ctx, "keyframe %d pyramid geometry differs from keyframe 0", k); return DSDTM_ERR_INVALID; }
    }
    for (int i = 0; i < m; ++i) {
        if (cand_kf[i] < 0 || cand_kf[i] >= n_kf || ref_level[i] < 0 || ref_level[i] >= p0.levels) {
            set_err(ctx, "candidate %d: keyframe %d / level %d out of range", i, cand_kf[i], ref_level[i]); return DSDTM_ERR_INVALID;
        }
    }
    const size_t M = (size_t)m;
    const size_t pitch = align_up(p0.bytes, 256);
    StageLayout lay;
    const size_t o_pyr = lay.take(pitch * (size_t)n_kf), o_tk = lay.take((size_t)n_kf * 96), o_rb = lay.take(M * 24), o_pw = lay.take(M * 24),
                 o_ck = lay.take(M * 4), o_rl = lay.take(M * 4), o_rp = lay.take(M * 8);
    const size_t in_bytes = lay.off;
    const size_t o_af = lay.take(M * 32), o_sl = lay.take(M * 4), o_pb = lay.take(M * 100), o_pp = lay.take(M * 64);
    const size_t total = lay.off;
    if (int rc = ensure_stage(ctx, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    for (int k = 0; k < n_kf; ++k) pack_pyramid(&kf_pyr[k], p0, h + o_pyr + pitch * (size_t)k);
    memcpy(h + o_tk, T_kf_w, (size_t)n_kf * 96);
    memcpy(h + o_rb, ref_bearing, M * 24);
    memcpy(h + o_pw, p_world, M * 24);
    memcpy(h + o_ck, cand_kf, M * 4);
    memcpy(h + o_rl, ref_level, M * 4);
    memcpy(h + o_rp, ref_px, M * 8);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const MatchColumns c = {(const double*)(d + o_tk), (const int32_t*)(d + o_ck), (const float*)(d + o_rp), (const int32_t*)(d + o_rl),
                            (const double*)(d + o_rb), (const double*)(d + o_pw), (double*)(d + o_af), (int32_t*)(d + o_sl), d + o_pb, d + o_pp,
                            nullptr, nullptr};
    LevelGeom lv[DSDTM_MAX_LEVELS];
    fill_levels(lv, p0, p0.levels);
    WarpKernelArgs a;
    fill_warp_args(a, c, cam, lv, p0.levels, m, n_kf, max_search_level);
    a.kf_pyr = d + o_pyr; a.kf_pitch = pitch;
    memcpy(a.T_cur_w, T_cur_w, 96);
    HIP_TRY(ctx, warp_launch(a, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + o_af, d + o_af, total - o_af, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (affine) memcpy(affine, h + o_af, M * 32);
    memcpy(search_level, h + o_sl, M * 4);
    memcpy(patch_border, h + o_pb, M * 100);
    memcpy(patch, h + o_pp, M * 64);
    return DSDTM_OK;
}

// ---- FindMatchDirect for M candidates on device-resident frames: warp prelude + Align2D, one call ----
extern "C" int dsdtm_match_candidates_frames(dsdtm_ctx* ctx, const dsdtm_frame* cur, const dsdtm_frame* const* kf, int n_kf,
                                             const dsdtm_camera* cam, const double* T_kf_w, const double T_cur_w[12],
                                             const int32_t* cand_kf, const float* ref_px, const int32_t* ref_level,
                                             const double* ref_bearing, const double* p_world, int max_search_level,
                                             int max_iters, int m, double* px_xy, int32_t* search_level, uint8_t* converged) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cur || !kf || n_kf <= 0 || n_kf > 4096 || !cam || !T_kf_w || !T_cur_w || m < 0 ||
        (m > 0 && (!cand_kf || !ref_px || !ref_level || !ref_bearing || !p_world || !px_xy || !search_level || !converged))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    if (m == 0) return DSDTM_OK;
    if (cur->owner != ctx) { set_err(ctx, "frame belongs to another context"); return DSDTM_ERR_INVALID; }
    const PackedPyr& p0 = cur->pl;
    unsigned long long frames_seq = cur->seq;
    for (int k = 0; k < n_kf; ++k) {
        if (!kf[k] || kf[k]->owner != ctx) { set_err(ctx, "keyframe %d: NULL or foreign frame", k); return DSDTM_ERR_INVALID; }
        if (kf[k]->seq > frames_seq) frames_seq = kf[k]->seq;
        const PackedPyr& pk = kf[k]->pl;
        if (!same_geometry(pk, p0)) { set_err(ctx, "keyframe %d pyramid geometry differs from the current frame", k); return DSDTM_ERR_INVALID; }
    }
    if (max_search_level < 0 || max_search_level >= p0.levels) { set_err(ctx, "max_search_level outside the pyramid"); return DSDTM_ERR_INVALID; }
    for (int i = 0; i < m; ++i) {
        if (cand_kf[i] < 0 || cand_kf[i] >= n_kf || ref_level[i] < 0 || ref_level[i] >= p0.levels) {
            set_err(ctx, "candidate %d: keyframe %d / level %d out of range", i, cand_kf[i], ref_level[i]); return DSDTM_ERR_INVALID;
        }
    }
    const size_t M = (size_t)m;
    StageLayout lay;
    const size_t o_ptr = lay.take((size_t)n_kf * sizeof(void*)), o_tk = lay.take((size_t)n_kf * 96), o_rb = lay.take(M * 24), o_pw = lay.take(M * 24),
                 o_ck = lay.take(M * 4), o_rl = lay.take(M * 4), o_rp = lay.take(M * 8),
                 o_px = lay.take(M * 16),                                       // in and out
                 o_sl = lay.take(M * 4), o_cv = lay.take(M),
                 o_af = lay.take(M * 32), o_pb = lay.take(M * 100), o_pp = lay.take(M * 64);   // device only
    if (int rc = ensure_stage(ctx, lay.off)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    for (int k = 0; k < n_kf; ++k) ((const uint8_t**)(h + o_ptr))[k] = kf[k]->d;
    memcpy(h + o_tk, T_kf_w, (size_t)n_kf * 96);
    memcpy(h + o_rb, ref_bearing, M * 24);
    memcpy(h + o_pw, p_world, M * 24);
    memcpy(h + o_ck, cand_kf, M * 4);
    memcpy(h + o_rl, ref_level, M * 4);
    memcpy(h + o_rp, ref_px, M * 8);
    memcpy(h + o_px, px_xy, M * 16);
    if (int rc = frames_consume(ctx, frames_seq, ctx->stream)) return rc;
    // Every input is read once per candidate and every result written once: the two kernels take them straight
    // from / to the pinned block (no copy operations around the launches); only the warped patches, which the
    // second kernel re-reads at every iteration, live in device memory.
    uint8_t* io = nullptr;
    if (int rc = pinned_device_ptr(ctx, &io)) return rc;
    const MatchColumns c = {(const double*)(io + o_tk), (const int32_t*)(io + o_ck), (const float*)(io + o_rp), (const int32_t*)(io + o_rl),
                            (const double*)(io + o_rb), (const double*)(io + o_pw), (double*)(d + o_af), (int32_t*)(io + o_sl), d + o_pb, d + o_pp,
                            (double*)(io + o_px), io + o_cv};
    LevelGeom lv[DSDTM_MAX_LEVELS];
    fill_levels(lv, p0, p0.levels);
    WarpKernelArgs a;
    A2DKernelArgs b;
    fill_match_args(a, b, c, cam, lv, p0.levels, m, n_kf, max_search_level, max_iters);
    a.kf_ptrs = (const uint8_t* const*)(io + o_ptr);
    memcpy(a.T_cur_w, T_cur_w, 96);
    b.cur_pyr = cur->d;
    if (int rc = launch_match(ctx, a, b, ctx->stream)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    frames_settle(ctx);
    memcpy(px_xy, h + o_px, M * 16);
    memcpy(search_level, h + o_sl, M * 4);
    memcpy(converged, h + o_cv, M);
    return DSDTM_OK;
}

// FindMatchDirect for the candidates of MANY current frames in one go (independent sequences): every pointer is a device
// pointer, nothing is copied, asynchronous on hip_stream.
extern "C" int dsdtm_match_candidates_batch_device(dsdtm_ctx* ctx, const uint8_t* cur_pyr, int n_frames, const uint8_t* kf_pyr, int n_kf,
                                                   size_t pyr_pitch, int levels, const int* width, const int* height, const int* stride,
                                                   const size_t* level_offset, const dsdtm_camera* cam, const double* T_kf_w,
                                                   const double* T_cur_w, const int32_t* cand_frame, const int32_t* cand_kf,
                                                   const float* ref_px, const int32_t* ref_level, const double* ref_bearing,
                                                   const double* p_world, int max_search_level, int max_iters, int m,
                                                   uint8_t* scratch, double* px_xy, int32_t* search_level, uint8_t* converged,
                                                   void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cur_pyr || !kf_pyr || n_frames <= 0 || n_kf <= 0 || !width || !height || !stride || !level_offset || !cam || !T_kf_w || !T_cur_w ||
        levels <= 0 || levels > DSDTM_MAX_LEVELS || m < 0 || (pyr_pitch & 3) ||
        (m > 0 && (!cand_frame || !cand_kf || !ref_px || !ref_level || !ref_bearing || !p_world || !scratch || !px_xy || !search_level || !converged))) {
        set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID;
    }
    if (max_search_level < 0 || max_search_level >= levels) { set_err(ctx, "max_search_level outside the pyramid"); return DSDTM_ERR_INVALID; }
    if (((size_t)scratch) & 15) { set_err(ctx, "scratch must be 16-byte aligned (the warped patches are written as whole dwords)"); return DSDTM_ERR_INVALID; }
    if (m == 0) return DSDTM_OK;
    const size_t M = (size_t)m;
    LevelGeom lv[DSDTM_MAX_LEVELS];
    if (int rc = check_levels(ctx, levels, width, height, stride, level_offset, pyr_pitch, "", "pyr_pitch", lv)) return rc;
    StageLayout lay;                                            // of `scratch`: M x 32, then M x 100, then M x 64 (256-byte aligned sections)
    const size_t o_af = lay.take(M * 32), o_pb = lay.take(M * 100), o_pp = lay.take(M * 64);
    const MatchColumns c = {T_kf_w, cand_kf, ref_px, ref_level, ref_bearing, p_world, (double*)(scratch + o_af), search_level, scratch + o_pb,
                            scratch + o_pp, px_xy, converged};
    WarpKernelArgs a;
    A2DKernelArgs b;
    fill_match_args(a, b, c, cam, lv, levels, m, n_kf, max_search_level, max_iters);
    a.kf_pyr = kf_pyr; a.kf_pitch = pyr_pitch; a.T_cur_w_arr = T_cur_w; a.cand_frame = cand_frame; a.n_frames = n_frames;
    b.cur_pyr = cur_pyr; b.frame = cand_frame; b.n_frames = n_frames; b.pyr_pitch = pyr_pitch;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_match(ctx, a, b, (hipStream_t)hip_stream);    // (fused: `scratch` is not touched)
}
extern "C" size_t dsdtm_match_candidates_scratch_bytes(int m) {
    StageLayout lay;                                            // (the sections of dsdtm_match_candidates_batch_device)
    const size_t M = m > 0 ? (size_t)m : 0;
    lay.take(M * 32); lay.take(M * 100); lay.take(M * 64);
    return lay.off;
}

// ---- Optimizer::PoseOptimization ---------------------------------------------------------------
extern "C" int dsdtm_pose_optimization_batch_device(dsdtm_ctx* ctx, int n_frames, int max_features,
                                                    const int32_t* n_features, const double* bearing,
                                                    const double* p_world, const int32_t* level, const uint8_t* use,
                                                    double* T_cur_w, const dsdtm_pose_opt_params* params,
                                                    double* residual_norm, dsdtm_pose_opt_summary* summary,
                                                    void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n_frames < 0 || max_features < 0 || !params || params->max_iterations < 0) {
        set_err(ctx, "bad argument"); return DSDTM_ERR_INVALID;
    }
    if (n_frames == 0) return DSDTM_OK;
    if (!T_cur_w || !summary || (max_features > 0 && (!bearing || !p_world || !level || !use || !residual_norm))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PoseOptArgs a;
    a.n_frames = n_frames; a.max_features = max_features; a.max_iterations = params->max_iterations;
    a.n_features = n_features; a.bearing = bearing; a.p_world = p_world; a.level = level; a.use = use;
    a.T_cur_w = T_cur_w; a.residual_norm = residual_norm; a.summary = summary;
    HIP_TRY(ctx, pose_opt_launch(a, (hipStream_t)hip_stream));
    return DSDTM_OK;
}

extern "C" int dsdtm_pose_optimization(dsdtm_ctx* ctx, const double* bearing, const double* p_world,
                                       const int32_t* level, const uint8_t* use, int n_features,
                                       double T_cur_w[12], const dsdtm_pose_opt_params* params,
                                       double* residual_norm, dsdtm_pose_opt_summary* summary) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!T_cur_w || !params || !summary || n_features < 0 ||
        (n_features > 0 && (!bearing || !p_world || !level || !use || !residual_norm))) {
        set_err(ctx, "NULL argument"); return DSDTM_ERR_INVALID;
    }
    for (int i = 0; i < n_features; ++i)
        if (use[i] && (level[i] < 0 || level[i] >= DSDTM_MAX_LEVELS)) {
            set_err(ctx, "feature %d: level %d out of range", i, level[i]); return DSDTM_ERR_INVALID;
        }
    const size_t N = (size_t)n_features;
    // (not a StageLayout: the columns are packed and this ladder rounds sizes, not offsets — `use` starts right behind `level`)
    size_t o = 0;
    const size_t o_T = o;   o += 12 * 8;                       // in/out
    const size_t o_sm = o;  o += align_up(sizeof(dsdtm_pose_opt_summary), 8);   // out
    const size_t o_rn = o;  o += N * 8;                        // out
    const size_t out_end = o;
    const size_t o_b = o;   o += N * 24;
    const size_t o_p = o;   o += N * 24;
    const size_t o_l = o;   o += N * 4;
    const size_t o_u = o;   o += align_up(N, 8);
    const size_t total = o;
    if (int rc = ensure_stage(ctx, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    memcpy(h + o_T, T_cur_w, 96);
    if (N) {
        memcpy(h + o_b, bearing, N * 24);
        memcpy(h + o_p, p_world, N * 24);
        memcpy(h + o_l, level, N * 4);
        memcpy(h + o_u, use, N);
    }
    // Up to 512 features the kernel keeps a lane's features in registers (pose_opt.hip, CACHED): every input is read once,
    // so it reads them straight from the pinned block and writes pose, summary and norms there — no copy operations
    // around the launch. Larger frames re-read their columns at every evaluation
    // and are copied to the device first.
    const bool zero_copy = n_features > 64 && n_features <= 512;
    if (zero_copy) {
        if (int rc = pinned_device_ptr(ctx, &d)) return rc;
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = dsdtm_pose_optimization_batch_device(ctx, 1, n_features, nullptr, (const double*)(d + o_b),
                                                      (const double*)(d + o_p), (const int32_t*)(d + o_l), d + o_u,
                                                      (double*)(d + o_T), params, (double*)(d + o_rn),
                                                      (dsdtm_pose_opt_summary*)(d + o_sm), ctx->stream)) return rc;
    if (!zero_copy) HIP_TRY(ctx, hipMemcpyAsync(h, d, out_end, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T_cur_w, h + o_T, 96);
    memcpy(summary, h + o_sm, sizeof(*summary));
    if (summary->n_residual_blocks > 0) memcpy(residual_norm, h + o_rn, (size_t)summary->n_residual_blocks * 8);
    return DSDTM_OK;
}

#ifdef DSDTM_DIAG
// ---- debug: device self-test of the FP64 building blocks (not in the public header) ------------
extern "C" int dsdtm_debug_selftest(dsdtm_ctx* ctx, const double* in, double* out, int n_cases) {
    if (!ctx || !in || !out || n_cases < 0) return DSDTM_ERR_INVALID;
    if (n_cases == 0) return DSDTM_OK;
    const size_t ib = align_up((size_t)n_cases * 33 * 8, 256), ob = (size_t)n_cases * 120 * 8;   // selftest.hip: SELFTEST_OUT
    if (int rc = ensure_stage(ctx, ib + ob)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* d = (uint8_t*)ctx->d_stage;
    memcpy(h, in, (size_t)n_cases * 33 * 8);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, ib, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, selftest_launch((const double*)d, (double*)(d + ib), n_cases, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + ib, d + ib, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, h + ib, ob);
    return DSDTM_OK;
}

// ---- debug: in-kernel stamps of the register kernel (diagnostic instantiation, never timed) ----
// stamps_dev: device buffer of n_pairs*8 uint64: [0] cycles the solver waited for the first pass of
// each level (precompute + pass), [1] waits of the later passes, [2] solve cycles, [3] iterations,
// [4] whole-block cycles, [5] s_memrealtime at the end, [6] s_memtime at the start.
extern "C" int dsdtm_debug_sparse_align_stamps(dsdtm_ctx* ctx, const dsdtm_batch_desc* b, const dsdtm_camera* cam,
                                               const dsdtm_align_params* prm, void* stamps_dev, void* hip_stream) {
    if (!ctx || !stamps_dev) return DSDTM_ERR_INVALID;
    g_stamp_out = stamps_dev;
    const int rc = dsdtm_sparse_align_batch_device(ctx, b, cam, prm, hip_stream);
    g_stamp_out = nullptr;
    return rc;
}

// ---- debug: a team launch whose last member is missing (not in the public header) ----------------
// The members that do run wait for a partner that never arrives: their bounded waits must run out, the pair must
// stop without hanging the device, and dsdtm_sparse_align_check must report it (tests/test_sparse_align_gpu.py).
extern "C" int dsdtm_debug_sparse_align_short_team(dsdtm_ctx* ctx, const dsdtm_batch_desc* b, const dsdtm_camera* cam,
                                                   const dsdtm_align_params* prm, void* hip_stream) {
    if (!ctx) return DSDTM_ERR_INVALID;
    g_team_drop_members = 1;
    const int rc = dsdtm_sparse_align_batch_device(ctx, b, cam, prm, hip_stream);
    g_team_drop_members = 0;
    return rc;
}

// tests: every team / two-member launch of the calling thread loses its last member until this is called with 0
extern "C" void dsdtm_debug_drop_team_members(int n) { g_team_drop_members = n > 0 ? 1 : 0; }

extern "C" int dsdtm_debug_occupancy(dsdtm_ctx* ctx, int variant) {
    if (!ctx) return DSDTM_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    return sparse_align_occupancy(variant);
}
#endif  // DSDTM_DIAG
