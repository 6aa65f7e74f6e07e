// addon_host.h — the host scaffold every add-on library (libdsdtm_amd_keyframe.so, libdsdtm_amd_motion.so) is written over: the
// context (device, stream, error text, one pinned and one device staging block), its create / destroy / last-error bodies, the error
// macros and the growth of the staging blocks. Header-only, and everything in it is `static`: each add-on has ONE host translation
// unit that includes it, so each library carries its own copy — and its own thread-local create-error text.
//
// An add-on's public context type stays opaque in its header and derives from the base in its *_api.cpp
// (`struct dsdtm_motion_ctx : dsdtm::AddonCtx {};`); its extern "C" create / destroy / last_error entries forward to the bodies here.
// Include it behind the add-on's own header (which brings the DSDTM_* status codes of include/dsdtm_amd.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

namespace dsdtm {

struct AddonCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    char err[512] = {0};
    void* h_pinned = nullptr;      // staging as the host sees it ...
    size_t h_cap = 0;
    void* d_stage = nullptr;       // ... and on the device
    size_t d_cap = 0;
};

static thread_local char g_create_err[512] = "";      // what *_last_error(NULL) answers: why the last create on this thread failed

static void set_err(AddonCtx* ctx, const char* fmt, ...) {
    char* dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

// (macros, so that the message names the call site)
#define HIP_TRY(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            dsdtm::set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return DSDTM_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)
// HIP_TRY behind the first enqueue: answered by the enclosing `fail` lambda (which waits for what was enqueued); needs `ctx` in scope
#define API_TRY(call)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) { dsdtm::set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return fail(DSDTM_ERR_HIP); } \
    } while (0)

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static const char* addon_last_error(const AddonCtx* ctx) { return ctx ? ctx->err : g_create_err; }

// `lib_name`: the library as its messages call it ("dsdtm_amd_motion")
template <class Ctx>
static int addon_create(const char* lib_name, int device, Ctx** out) {
    if (!out) return DSDTM_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err(nullptr, "no HIP device visible (%s); %s has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0", lib_name);
        return DSDTM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { set_err(nullptr, "device %d out of range (%d visible)", device, n); return DSDTM_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_err(nullptr, "hipGetDeviceProperties(%d) failed", device); return DSDTM_ERR_NO_DEVICE; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "device %d is %s; this library contains gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return DSDTM_ERR_NO_DEVICE;
    }
    Ctx* ctx = new (std::nothrow) Ctx();
    if (!ctx) return DSDTM_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        set_err(nullptr, "hipSetDevice/hipStreamCreate failed on device %d", device);
        delete ctx;
        return DSDTM_ERR_HIP;
    }
    *out = ctx;
    return DSDTM_OK;
}

template <class Ctx>
static void addon_destroy(Ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    delete ctx;
}

// Both staging blocks at least this large (the two may differ: a device block can hold what is never copied back). A block that must
// grow is freed first and re-allocated at the request plus a quarter, rounded up to 64 KiB; a failed allocation leaves its cap at 0.
static int ensure_stage(AddonCtx* ctx, size_t h_bytes, size_t d_bytes) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (h_bytes > ctx->h_cap) {
        if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
        ctx->h_pinned = nullptr; ctx->h_cap = 0;
        const size_t cap = align_up(h_bytes + h_bytes / 4, 1 << 16);
        HIP_TRY(ctx, hipHostMalloc(&ctx->h_pinned, cap, hipHostMallocDefault));
        ctx->h_cap = cap;
    }
    if (d_bytes > ctx->d_cap) {
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        ctx->d_stage = nullptr; ctx->d_cap = 0;
        const size_t cap = align_up(d_bytes + d_bytes / 4, 1 << 16);
        HIP_TRY(ctx, hipMalloc(&ctx->d_stage, cap));
        ctx->d_cap = cap;
    }
    return DSDTM_OK;
}

}  // namespace dsdtm
