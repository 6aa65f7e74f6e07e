// undistort_api.cpp — the C ABI of include/dsdtm_amd_undistort.h (libdsdtm_amd_undistort.so): checks, staging, launch (the context:
// addon_host.h).
//
// dsdtm_undistort_frames checks every desc, lays ONE block out (the frames' records, every pageable source packed, then every host
// destination packed), fills the pinned side, moves the front with a single hipMemcpyAsync, launches undistort.hip's kernel once for all
// frames, copies the host destinations' part back with one copy and waits once; the caller's host destinations are written only after
// the wait succeeded. There is no CPU compute path here (the host evaluation of the same rules is host/dsdtm_undistort_host.hpp, which
// needs no library).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "undistort.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_undistort_ctx : dsdtm::AddonCtx {};      // (staging: the upload and the read-back, at the same offsets on both sides)
struct dsdtm_undistort_map {
    int device = 0;
    int w = 0, h = 0;
    int32_t* d_xy = nullptr;                          // device: w * h pairs (X, Y)
};

extern "C" const char* dsdtm_undistort_last_error(const dsdtm_undistort_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_undistort_create(int device, dsdtm_undistort_ctx** out) { return addon_create("dsdtm_amd_undistort", device, out); }
extern "C" void dsdtm_undistort_destroy(dsdtm_undistort_ctx* ctx) { addon_destroy(ctx); }

// what is wrong with the camera or the distortion, or nullptr (`sides`: the map's width and height are checked too)
static const char* check_model(const dsdtm_camera* cam, const float* dist, bool sides, UndistortModel* m) {
    if (!cam) return "cam is NULL";
    if (!dist) return "dist is NULL";
    if (sides && (cam->width < DSDTM_UNDISTORT_MIN_SIDE || cam->width > DSDTM_UNDISTORT_MAX_SIDE)) return "cam: width out of range";
    if (sides && (cam->height < DSDTM_UNDISTORT_MIN_SIDE || cam->height > DSDTM_UNDISTORT_MAX_SIDE)) return "cam: height out of range";
    if (!std::isfinite(cam->fx) || !(cam->fx > 0.0f)) return "cam: fx is not a finite number above 0";
    if (!std::isfinite(cam->fy) || !(cam->fy > 0.0f)) return "cam: fy is not a finite number above 0";
    if (!std::isfinite(cam->cx)) return "cam: cx is not finite";
    if (!std::isfinite(cam->cy)) return "cam: cy is not finite";
    static const char* const names[5] = {"dist: k1 is not finite", "dist: k2 is not finite", "dist: p1 is not finite", "dist: p2 is not finite",
                                         "dist: k3 is not finite"};
    for (int i = 0; i < 5; ++i) if (!std::isfinite(dist[i])) return names[i];
    m->fx = cam->fx; m->fy = cam->fy; m->cx = cam->cx; m->cy = cam->cy;
    m->k1 = dist[0]; m->k2 = dist[1]; m->p1 = dist[2]; m->p2 = dist[3]; m->k3 = dist[4];
    return nullptr;
}

static bool capturing(dsdtm_undistort_ctx* ctx) {      // (every entry allocates or waits: neither can be part of a capture)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return cs != hipStreamCaptureStatusNone;
}

extern "C" int dsdtm_undistort_map_create(dsdtm_undistort_ctx* ctx, const dsdtm_camera* cam, const float dist[5], dsdtm_undistort_map** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "undistort_map_create: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    UndistortModel m;
    if (const char* bad = check_model(cam, dist, true, &m)) { set_err(ctx, "undistort_map_create: %s", bad); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "undistort_map_create: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    dsdtm_undistort_map* map = new (std::nothrow) dsdtm_undistort_map();
    if (!map) { set_err(ctx, "undistort_map_create: out of memory"); return DSDTM_ERR_NOMEM; }
    map->device = ctx->device; map->w = cam->width; map->h = cam->height;
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(ctx->stream);
        if (map->d_xy) (void)hipFree(map->d_xy);
        delete map;
        return rc;
    };
    void* d = nullptr;
    API_TRY(hipMalloc(&d, (size_t)map->w * (size_t)map->h * 8));
    map->d_xy = (int32_t*)d;
    API_TRY(undistort_map_launch(m, map->w, map->h, map->d_xy, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    *out = map;
    return DSDTM_OK;
}

extern "C" void dsdtm_undistort_map_destroy(dsdtm_undistort_map* map) {
    if (!map) return;
    (void)hipSetDevice(map->device);
    if (map->d_xy) (void)hipFree(map->d_xy);          // (waits for the device)
    delete map;
}

extern "C" int dsdtm_undistort_map_read(dsdtm_undistort_ctx* ctx, const dsdtm_undistort_map* map, int32_t* xy_out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!map || !xy_out) { set_err(ctx, "undistort_map_read: %s is NULL", !map ? "map" : "xy_out"); return DSDTM_ERR_INVALID; }
    if (map->device != ctx->device) { set_err(ctx, "undistort_map_read: the map lies on device %d, the context on device %d", map->device, ctx->device); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "undistort_map_read: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    const size_t bytes = (size_t)map->w * (size_t)map->h * 8;
    if (int rc = ensure_stage(ctx, bytes, 0)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, map->d_xy, bytes, hipMemcpyDeviceToHost, ctx->stream));
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    API_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(xy_out, ctx->h_pinned, bytes);
    return DSDTM_OK;
}

// ---- where a caller's image lies: THE rule for the four images of a desc
enum { MEM_PAGEABLE = 0, MEM_PINNED = 1, MEM_DEVICE = 2, MEM_OTHER_DEVICE = -1 };
static int array_memory(const dsdtm_undistort_ctx* ctx, const void* p) {
    hipPointerAttribute_t pa_;
    if (hipPointerGetAttributes(&pa_, p) != hipSuccess) { (void)hipGetLastError(); return MEM_PAGEABLE; }    // (an ordinary host pointer: not an error)
    if (pa_.type == hipMemoryTypeDevice) return pa_.device == ctx->device ? MEM_DEVICE : MEM_OTHER_DEVICE;
    if (pa_.type == hipMemoryTypeHost) return MEM_PINNED;
    return MEM_PAGEABLE;
}

enum { IMG_GRAY_SRC = 0, IMG_GRAY_DST = 1, IMG_DEPTH_SRC = 2, IMG_DEPTH_DST = 3 };
static const char* const IMG_NAME[4] = {"gray_src", "gray_dst", "depth_src", "depth_dst"};
struct Image {
    const void* p = nullptr;
    size_t elem = 1, stride = 0;      // bytes per element; the caller's stride in elements
    int mem = MEM_PAGEABLE;
    size_t off = 0;                   // where in the block: a pageable source, a host destination (packed: stride = width)
};
struct FramePlan { Image img[4]; };
struct Extent { uintptr_t lo, hi; int frame, what; };

extern "C" int dsdtm_undistort_frames(dsdtm_undistort_ctx* ctx, int n, const dsdtm_undistort_desc* descs) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_UNDISTORT_MAX_FRAMES) { set_err(ctx, "undistort_frames: n = %d outside 0..%d", n, DSDTM_UNDISTORT_MAX_FRAMES); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "undistort_frames: descs is NULL"); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "undistort_frames: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every desc is checked before anything is enqueued; the block's layout on the way:
    //   records | every pageable source, packed || every host destination, packed
    const size_t N = (size_t)n;
    std::vector<FramePlan> plan(N);
    std::vector<Extent> extents;
    extents.reserve(4 * N);
    int max_w = 0, max_h = 0;
    size_t o = align_up(N * sizeof(UndistortFrameDev), 256);
    for (int t = 0; t < n; ++t) {
        const dsdtm_undistort_desc& d = descs[t];
        FramePlan& p = plan[(size_t)t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (d.map->device != ctx->device) bad = "map lies on another device";
        else if (!d.gray_src) bad = "gray_src is NULL";
        else if (!d.gray_dst) bad = "gray_dst is NULL";
        else if (d.gray_src_stride < d.map->w) bad = "gray_src_stride below width";
        else if (d.gray_dst_stride < d.map->w) bad = "gray_dst_stride below width";
        else if (!d.depth_src != !d.depth_dst) bad = !d.depth_src ? "depth_src is NULL but depth_dst is not" : "depth_dst is NULL but depth_src is not";
        else if (d.depth_src && d.depth_src_stride < d.map->w) bad = "depth_src_stride below width";
        else if (d.depth_src && d.depth_dst_stride < d.map->w) bad = "depth_dst_stride below width";
        if (bad) { set_err(ctx, "undistort_frames: frame %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        const size_t W = (size_t)d.map->w, H = (size_t)d.map->h;
        max_w = std::max(max_w, d.map->w); max_h = std::max(max_h, d.map->h);
        const void* ptr[4] = {d.gray_src, d.gray_dst, d.depth_src, d.depth_dst};
        const int32_t stride[4] = {d.gray_src_stride, d.gray_dst_stride, d.depth_src_stride, d.depth_dst_stride};
        for (int k = 0; k < 4; ++k) {
            if (!ptr[k]) continue;
            Image& im = p.img[k];
            im.p = ptr[k]; im.elem = k >= IMG_DEPTH_SRC ? 2 : 1; im.stride = (size_t)stride[k];
            im.mem = array_memory(ctx, ptr[k]);
            if (im.mem == MEM_OTHER_DEVICE) { set_err(ctx, "undistort_frames: frame %d: %s lies in another device's memory", t, IMG_NAME[k]); return DSDTM_ERR_INVALID; }
            const bool is_dst = k == IMG_GRAY_DST || k == IMG_DEPTH_DST;
            if (!is_dst && im.mem == MEM_PAGEABLE) { im.off = o; o = align_up(o + W * H * im.elem, 16); }
            const uintptr_t lo = (uintptr_t)ptr[k];
            extents.push_back(Extent{lo, lo + ((H - 1) * im.stride + W) * im.elem, t, k});
        }
    }
    const size_t upload = align_up(o, 256);
    o = upload;
    for (int t = 0; t < n; ++t)
        for (int k : {IMG_GRAY_DST, IMG_DEPTH_DST}) {
            Image& im = plan[(size_t)t].img[k];
            if (!im.p || im.mem == MEM_DEVICE) continue;
            im.off = o; o = align_up(o + (size_t)descs[t].map->w * (size_t)descs[t].map->h * im.elem, 16);
        }
    const size_t total = o, back = total - upload;
    {   // no destination's extent meets a source's or another destination's (a sweep over the extents in address order)
        std::sort(extents.begin(), extents.end(), [](const Extent& a, const Extent& b) { return a.lo < b.lo; });
        const Extent* far_dst = nullptr;      // the destination / the image of any kind that reaches furthest so far
        const Extent* far_any = nullptr;
        for (const Extent& e : extents) {
            const bool is_dst = e.what == IMG_GRAY_DST || e.what == IMG_DEPTH_DST;
            const Extent* hit = is_dst ? far_any : far_dst;
            if (hit && e.lo < hit->hi) {
                const Extent& dst = is_dst ? e : *hit;
                const Extent& other = is_dst ? *hit : e;
                set_err(ctx, "undistort_frames: frame %d: %s overlaps %s of frame %d", dst.frame, IMG_NAME[dst.what], IMG_NAME[other.what], other.frame);
                return DSDTM_ERR_INVALID;
            }
            if (is_dst && (!far_dst || e.hi > far_dst->hi)) far_dst = &e;
            if (!far_any || e.hi > far_any->hi) far_any = &e;
        }
    }
    if (int rc = ensure_stage(ctx, total, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    for (int t = 0; t < n; ++t) {
        const dsdtm_undistort_desc& d = descs[t];
        const FramePlan& p = plan[(size_t)t];
        const size_t W = (size_t)d.map->w, H = (size_t)d.map->h;
        const void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t stride[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            const Image& im = p.img[k];
            if (!im.p) continue;
            const bool is_dst = k == IMG_GRAY_DST || k == IMG_DEPTH_DST;
            stride[k] = im.stride;
            if (im.mem == MEM_DEVICE) dev[k] = im.p;
            else if (is_dst) { dev[k] = g + im.off; stride[k] = W; }                          // read back, packed
            else if (im.mem == MEM_PINNED) {
                void* v = nullptr;
                HIP_TRY(ctx, hipHostGetDevicePointer(&v, const_cast<void*>(im.p), 0));
                dev[k] = v;
            } else {                                                                          // pageable: packed into the upload
                const size_t row = W * im.elem;
                for (size_t r = 0; r < H; ++r) memcpy(h + im.off + r * row, (const uint8_t*)im.p + r * im.stride * im.elem, row);
                dev[k] = g + im.off; stride[k] = W;
            }
        }
        UndistortFrameDev f;
        memset(&f, 0, sizeof f);
        f.map = d.map->d_xy; f.w = d.map->w; f.h = d.map->h;
        f.gray_src = (const uint8_t*)dev[IMG_GRAY_SRC]; f.gray_dst = (uint8_t*)const_cast<void*>(dev[IMG_GRAY_DST]);
        f.depth_src = (const uint16_t*)dev[IMG_DEPTH_SRC]; f.depth_dst = (uint16_t*)const_cast<void*>(dev[IMG_DEPTH_DST]);
        f.gray_src_stride = (int32_t)stride[IMG_GRAY_SRC]; f.gray_dst_stride = (int32_t)stride[IMG_GRAY_DST];
        f.depth_src_stride = (int32_t)stride[IMG_DEPTH_SRC]; f.depth_dst_stride = (int32_t)stride[IMG_DEPTH_DST];
        memcpy(h + (size_t)t * sizeof f, &f, sizeof f);
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, upload, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(undistort_frames_launch((const UndistortFrameDev*)g, n, max_w, max_h, ctx->stream));
    if (back) API_TRY(hipMemcpyAsync(h + upload, g + upload, back, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t)
        for (int k : {IMG_GRAY_DST, IMG_DEPTH_DST}) {
            const Image& im = plan[(size_t)t].img[k];
            if (!im.p || im.mem == MEM_DEVICE) continue;
            const size_t row = (size_t)descs[t].map->w * im.elem;
            for (size_t r = 0; r < (size_t)descs[t].map->h; ++r) memcpy((uint8_t*)const_cast<void*>(im.p) + r * im.stride * im.elem, h + im.off + r * row, row);
        }
    return DSDTM_OK;
}

extern "C" int dsdtm_undistort_points(dsdtm_undistort_ctx* ctx, const dsdtm_camera* cam, const float dist[5], int n, const float* px_in,
                                      const uint8_t* skip, float* px_out, double* bearing_out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    UndistortModel m;
    if (const char* bad = check_model(cam, dist, false, &m)) { set_err(ctx, "undistort_points: %s", bad); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_UNDISTORT_MAX_POINTS) { set_err(ctx, "undistort_points: n = %d outside 0..%d", n, DSDTM_UNDISTORT_MAX_POINTS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!px_in || !px_out || !bearing_out) { set_err(ctx, "undistort_points: %s is NULL", !px_in ? "px_in" : !px_out ? "px_out" : "bearing_out"); return DSDTM_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(px_in[2 * i]) || !std::isfinite(px_in[2 * i + 1])) { set_err(ctx, "undistort_points: px_in is not finite at index %d", i); return DSDTM_ERR_INVALID; }
    if (capturing(ctx)) { set_err(ctx, "undistort_points: not inside a stream capture"); return DSDTM_ERR_INVALID; }
    // the block: px_in | skip || px_out | bearing
    const size_t N = (size_t)n, in_px = 0, in_skip = align_up(N * 8, 16), upload = align_up(in_skip + N, 256);
    const size_t out_px = upload, out_bearing = align_up(out_px + N * 8, 16), total = out_bearing + N * 24;
    if (int rc = ensure_stage(ctx, total, total)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h + in_px, px_in, N * 8);
    if (skip) memcpy(h + in_skip, skip, N); else memset(h + in_skip, 0, N);
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, upload, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(undistort_points_launch(m, cam->fx, cam->fy, cam->cx, cam->cy, n, (const float*)(g + in_px), g + in_skip, (float*)(g + out_px),
                                    (double*)(g + out_bearing), ctx->stream));
    API_TRY(hipMemcpyAsync(h + upload, g + upload, total - upload, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    const uint8_t* sk = h + in_skip;      // (the call's own copy: px_out may be px_in, and skip may be NULL)
    memcpy(px_out, h + out_px, N * 8);
    for (size_t i = 0; i < N; ++i) if (!sk[i]) memcpy(bearing_out + 3 * i, h + out_bearing + 24 * i, 24);
    return DSDTM_OK;
}
