// clahe_api.cpp — the C ABI of include/dsdtm_amd_clahe.h (libdsdtm_amd_clahe.so): checks, staging, launch (the context:
// addon_host.h).
//
// dsdtm_clahe_apply_batch checks every desc, lays ONE block out (the frames' records, every pageable source packed, then what is read
// back: the tables somebody asked for and every host destination packed; behind that, on the device only, the tables nobody asked
// for), fills the pinned side, moves the front with a single hipMemcpyAsync, launches clahe.hip's two kernels once each for all frames,
// copies the read-back part with one copy and waits once; the caller's host memory is written only after the wait succeeded. E1 and E2
// are evaluated here by clahe_geometry of host/dsdtm_clahe_host.hpp (one definition for the library and the host path). There is no
// CPU compute path here (the host evaluation of the same rules is clahe_host of that header, which needs no library).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "clahe.h"
#include "addon_host.h"
#include "../host/dsdtm_clahe_host.hpp"

using namespace dsdtm;

struct dsdtm_clahe_ctx : dsdtm::AddonCtx {};      // (staging: the upload and the read-back, at the same offsets on both sides)

extern "C" const char* dsdtm_clahe_last_error(const dsdtm_clahe_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_clahe_create(int device, dsdtm_clahe_ctx** out) { return addon_create("dsdtm_amd_clahe", device, out); }
extern "C" void dsdtm_clahe_destroy(dsdtm_clahe_ctx* ctx) { addon_destroy(ctx); }

static bool capturing(dsdtm_clahe_ctx* ctx) {      // (every entry allocates or waits: neither can be part of a capture)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return cs != hipStreamCaptureStatusNone;
}

// ---- where a caller's array lies: THE rule for the three arrays of a desc (as in undistort_api.cpp)
enum { MEM_PAGEABLE = 0, MEM_PINNED = 1, MEM_DEVICE = 2, MEM_OTHER_DEVICE = -1 };
static int array_memory(const dsdtm_clahe_ctx* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return MEM_PAGEABLE; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? MEM_DEVICE : MEM_OTHER_DEVICE;
    if (pa_.type == hipMemoryTypeHost) return MEM_PINNED;
    return MEM_PAGEABLE;
}

enum { ARR_SRC = 0, ARR_DST = 1, ARR_LUT = 2 };
static const char* const ARR_NAME[3] = {"src", "dst", "lut_out"};
struct FramePlan {
    DSDTM::ClaheGeometry g;
    int src_mem = MEM_PAGEABLE, dst_mem = MEM_PAGEABLE;
    size_t src_off = 0, dst_off = 0, lut_off = 0;      // where in the block: a pageable source, a host destination (both packed), the tables
    size_t lut_bytes = 0;
};
struct Extent { uintptr_t lo, hi; int frame, what; };

// the body of the three entries; luts_only: dsdtm_clahe_luts (`who` names the entry in messages)
static int run(dsdtm_clahe_ctx* ctx, const char* who, int n, const dsdtm_clahe_desc* descs, bool luts_only, bool batch) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_CLAHE_MAX_FRAMES) { set_err(ctx, "%s: n = %d outside 0..%d", who, n, DSDTM_CLAHE_MAX_FRAMES); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "%s: %s is NULL", who, batch ? "descs" : "desc"); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "%s: not inside a stream capture", who); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   records | every pageable source, packed || tables asked for | every host destination, packed ||| (device only) the other tables
    const size_t N = (size_t)n;
    std::vector<FramePlan> plan(N);
    std::vector<Extent> extents;
    extents.reserve(3 * N);
    int max_w = 0, max_tile_h = 0, max_tiles = 0, max_tiles_y = 0;
    size_t o = align_up(N * sizeof(ClaheFrameDev), 256);
    for (int t = 0; t < n; ++t) {
        const dsdtm_clahe_desc& d = descs[t];
        FramePlan& p = plan[(size_t)t];
        const char* bad = nullptr;
        if (d.width < DSDTM_CLAHE_MIN_SIDE || d.width > DSDTM_CLAHE_MAX_SIDE) bad = "width out of range";
        else if (d.height < DSDTM_CLAHE_MIN_SIDE || d.height > DSDTM_CLAHE_MAX_SIDE) bad = "height out of range";
        else if (d.tiles_x < 0 || d.tiles_x > DSDTM_CLAHE_MAX_TILES) bad = "tiles_x out of range";
        else if (d.tiles_y < 0 || d.tiles_y > DSDTM_CLAHE_MAX_TILES) bad = "tiles_y out of range";
        else if (!std::isfinite(d.clip_limit) || d.clip_limit < 0.0) bad = "clip_limit is not a finite number at or above 0";
        else if (!d.src) bad = "src is NULL";
        else if (!luts_only && !d.dst) bad = "dst is NULL";
        else if (luts_only && !d.lut_out) bad = "lut_out is NULL";
        else if (d.src_stride < d.width) bad = "src_stride below width";
        else if (!luts_only && d.dst_stride < d.width) bad = "dst_stride below width";
        if (bad) { set_err(ctx, "%s: desc %d: %s", who, t, bad); return DSDTM_ERR_INVALID; }
        p.g = DSDTM::clahe_geometry(d.width, d.height, d.clip_limit, d.tiles_x, d.tiles_y);
        p.lut_bytes = (size_t)p.g.tiles_x * (size_t)p.g.tiles_y * 256;
        const size_t W = (size_t)d.width, H = (size_t)d.height;
        max_w = std::max(max_w, d.width); max_tile_h = std::max(max_tile_h, p.g.tile_h);
        max_tiles = std::max(max_tiles, p.g.tiles_x * p.g.tiles_y); max_tiles_y = std::max(max_tiles_y, p.g.tiles_y);
        const void* ptr[3] = {d.src, luts_only ? nullptr : d.dst, d.lut_out};
        const size_t bytes[3] = {(H - 1) * (size_t)d.src_stride + W, luts_only ? 0 : (H - 1) * (size_t)d.dst_stride + W, p.lut_bytes};
        for (int k = 0; k < 3; ++k) {
            if (!ptr[k]) continue;
            const int mem = array_memory(ctx, ptr[k]);
            if (mem == MEM_OTHER_DEVICE) { set_err(ctx, "%s: desc %d: %s lies in another device's memory", who, t, ARR_NAME[k]); return DSDTM_ERR_INVALID; }
            if (k == ARR_LUT && mem == MEM_DEVICE) { set_err(ctx, "%s: desc %d: lut_out lies in device memory (it is a host pointer)", who, t); return DSDTM_ERR_INVALID; }
            if (k == ARR_SRC) { p.src_mem = mem; if (mem == MEM_PAGEABLE) { p.src_off = o; o = align_up(o + W * H, 16); } }
            if (k == ARR_DST) p.dst_mem = mem;
            const uintptr_t lo = (uintptr_t)ptr[k];
            extents.push_back(Extent{lo, lo + bytes[k], t, k});
        }
    }
    const size_t upload = align_up(o, 256);
    o = upload;
    for (int t = 0; t < n; ++t)
        if (descs[t].lut_out) { plan[(size_t)t].lut_off = o; o += plan[(size_t)t].lut_bytes; }          // (multiples of 256)
    if (!luts_only)
        for (int t = 0; t < n; ++t)
            if (plan[(size_t)t].dst_mem != MEM_DEVICE) { plan[(size_t)t].dst_off = o; o = align_up(o + (size_t)descs[t].width * (size_t)descs[t].height, 16); }
    const size_t total = o, back = total - upload;
    o = align_up(o, 256);
    for (int t = 0; t < n; ++t)
        if (!descs[t].lut_out) { plan[(size_t)t].lut_off = o; o += plan[(size_t)t].lut_bytes; }
    const size_t device_total = o;
    {   // no destination's extent meets a source's or another destination's (a sweep over the extents in address order)
        std::sort(extents.begin(), extents.end(), [](const Extent& a, const Extent& b) { return a.lo < b.lo; });
        const Extent* far_dst = nullptr;      // the destination / the array of any kind that reaches furthest so far
        const Extent* far_any = nullptr;
        for (const Extent& e : extents) {
            const bool is_dst = e.what != ARR_SRC;
            const Extent* hit = is_dst ? far_any : far_dst;
            if (hit && e.lo < hit->hi) {
                const Extent& dst = is_dst ? e : *hit;
                const Extent& other = is_dst ? *hit : e;
                set_err(ctx, "%s: desc %d: %s overlaps %s of desc %d", who, dst.frame, ARR_NAME[dst.what], ARR_NAME[other.what], other.frame);
                return DSDTM_ERR_INVALID;
            }
            if (is_dst && (!far_dst || e.hi > far_dst->hi)) far_dst = &e;
            if (!far_any || e.hi > far_any->hi) far_any = &e;
        }
    }
    if (int rc = ensure_stage(ctx, total, device_total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    for (int t = 0; t < n; ++t) {
        const dsdtm_clahe_desc& d = descs[t];
        const FramePlan& p = plan[(size_t)t];
        const size_t W = (size_t)d.width, H = (size_t)d.height;
        ClaheFrameDev f;
        memset(&f, 0, sizeof f);
        f.w = d.width; f.h = d.height; f.src_stride = d.src_stride; f.dst_stride = d.dst_stride;
        if (p.src_mem == MEM_DEVICE) f.src = d.src;
        else if (p.src_mem == MEM_PINNED) {
            void* v = nullptr;
            HIP_TRY(ctx, hipHostGetDevicePointer(&v, const_cast<uint8_t*>(d.src), 0));
            f.src = (const uint8_t*)v;
        } else {                                                                              // pageable: packed into the upload
            for (size_t r = 0; r < H; ++r) memcpy(h + p.src_off + r * W, d.src + r * (size_t)d.src_stride, W);
            f.src = g + p.src_off; f.src_stride = d.width;
        }
        if (luts_only) { f.dst = nullptr; f.dst_stride = 0; }
        else if (p.dst_mem == MEM_DEVICE) f.dst = d.dst;
        else { f.dst = g + p.dst_off; f.dst_stride = d.width; }                               // read back, packed
        f.luts = g + p.lut_off;
        f.tiles_x = p.g.tiles_x; f.tiles_y = p.g.tiles_y; f.tile_w = p.g.tile_w; f.tile_h = p.g.tile_h;
        f.clip = p.g.clip; f.scale = p.g.scale; f.inv_tw = p.g.inv_tw; f.inv_th = p.g.inv_th;
        memcpy(h + (size_t)t * sizeof f, &f, sizeof f);
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, upload, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(clahe_luts_launch((const ClaheFrameDev*)g, n, max_tiles, ctx->stream));
    if (!luts_only) API_TRY(clahe_interp_launch((const ClaheFrameDev*)g, n, max_w, max_tile_h, max_tiles_y, ctx->stream));
    if (back) API_TRY(hipMemcpyAsync(h + upload, g + upload, back, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        const dsdtm_clahe_desc& d = descs[t];
        const FramePlan& p = plan[(size_t)t];
        if (d.lut_out) memcpy(d.lut_out, h + p.lut_off, p.lut_bytes);
        if (luts_only || p.dst_mem == MEM_DEVICE) continue;
        const size_t W = (size_t)d.width;
        for (size_t r = 0; r < (size_t)d.height; ++r) memcpy(d.dst + r * (size_t)d.dst_stride, h + p.dst_off + r * W, W);
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_clahe_apply_batch(dsdtm_clahe_ctx* ctx, int n, const dsdtm_clahe_desc* descs) { return run(ctx, "clahe_apply_batch", n, descs, false, true); }
extern "C" int dsdtm_clahe_apply(dsdtm_clahe_ctx* ctx, const dsdtm_clahe_desc* desc) { return run(ctx, "clahe_apply", 1, desc, false, false); }
extern "C" int dsdtm_clahe_luts(dsdtm_clahe_ctx* ctx, const dsdtm_clahe_desc* desc) { return run(ctx, "clahe_luts", 1, desc, true, false); }
