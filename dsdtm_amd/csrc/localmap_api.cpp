// localmap_api.cpp — the C ABI of include/dsdtm_amd_localmap.h (libdsdtm_amd_localmap.so): the resident map, its updates, the checks
// and the packing of a select (the context: addon_host.h).
//
// A map is three device arrays (points, keyframe records, the slot pool) and, on the host, only what the checks need: the counts
// and each keyframe's slot count and offset. An UPDATE is staged in the context's pinned block — handed out piece by piece, so
// that an update never overwrites what an earlier one has staged and the stream has not yet read; the stream is waited for only
// when the block is full — then moved by one copy into the device staging block and applied by one launch: an update that
// fails at any HIP call has changed nothing. A SELECT is one upload (the descs with their poses), the two launches of
// localmap.hip, one read-back of the results of all descs and one wait. There is no CPU compute path here (the host
// evaluation of the same rules is select_local_map_host of host/dsdtm_localmap_host.hpp, which needs no library).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "localmap.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_localmap {
    LmPointDev* d_points = nullptr;
    LmKeyframeDev* d_kfs = nullptr;
    int32_t* d_slots = nullptr;
    int64_t cap_points = 0, cap_kfs = 0, cap_slots = 0;     // elements allocated
    int64_t n_points = 0, n_kfs = 0, n_slots = 0;           // elements in use, as of the last update enqueued
    std::vector<int32_t> kf_n_slots;                        // per keyframe: what keyframe_write and map_read check against
    std::vector<int64_t> kf_slot_off;
};

struct dsdtm_localmap_ctx : dsdtm::AddonCtx {
    std::vector<dsdtm_localmap*> maps;
    std::vector<void*> retired;     // device arrays a map has outgrown: freed once the stream has been waited for
    size_t h_used = 0;              // bytes of the pinned block handed out since the stream was last waited for
};

static void release_retired(dsdtm_localmap_ctx* ctx) {
    for (void* p : ctx->retired) (void)hipFree(p);
    ctx->retired.clear();
}

// the stream has run dry: every staged byte has been read, every outgrown array has been passed
static void stream_idle(dsdtm_localmap_ctx* ctx) {
    ctx->h_used = 0;
    release_retired(ctx);
}

static void free_map(dsdtm_localmap* m) {
    if (m->d_points) (void)hipFree(m->d_points);
    if (m->d_kfs) (void)hipFree(m->d_kfs);
    if (m->d_slots) (void)hipFree(m->d_slots);
    delete m;
}

extern "C" const char* dsdtm_localmap_last_error(const dsdtm_localmap_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_localmap_create(int device, dsdtm_localmap_ctx** out) { return addon_create("dsdtm_amd_localmap", device, out); }
extern "C" void dsdtm_localmap_destroy(dsdtm_localmap_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (dsdtm_localmap* m : ctx->maps) free_map(m);
    ctx->maps.clear();
    release_retired(ctx);
    addon_destroy(ctx);
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

static bool owns(const dsdtm_localmap_ctx* ctx, const dsdtm_localmap* map) {
    return map && std::find(ctx->maps.begin(), ctx->maps.end(), map) != ctx->maps.end();
}

extern "C" int dsdtm_localmap_map_create(dsdtm_localmap_ctx* ctx, dsdtm_localmap** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "map_create: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    dsdtm_localmap* m = new (std::nothrow) dsdtm_localmap();
    if (!m) { set_err(ctx, "map_create: out of host memory"); return DSDTM_ERR_NOMEM; }
    ctx->maps.push_back(m);         // (the device arrays come with the first update that needs them)
    *out = m;
    return DSDTM_OK;
}

extern "C" void dsdtm_localmap_map_destroy(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map) {
    if (!ctx || !owns(ctx, map)) return;
    (void)hipSetDevice(ctx->device);
    if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx);      // (updates of this map may still be on their way)
    ctx->maps.erase(std::find(ctx->maps.begin(), ctx->maps.end(), map));
    free_map(map);
}

// `bytes` of the pinned block that no earlier update still needs
static int pinned_reserve(dsdtm_localmap_ctx* ctx, size_t bytes, uint8_t** out) {
    bytes = align_up(bytes, 256);
    if (ctx->h_used + bytes > ctx->h_cap) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        stream_idle(ctx);
        if (bytes > ctx->h_cap)
            if (int rc = ensure_stage(ctx, std::max(bytes, (size_t)1 << 20), 0)) return rc;
    }
    *out = (uint8_t*)ctx->h_pinned + ctx->h_used;
    ctx->h_used += bytes;
    return DSDTM_OK;
}

// `bytes` of the device staging block. A block that must grow is freed by ensure_stage, and an earlier update's copy into it or
// launch reading it may still be queued: the stream is waited for first, explicitly, rather than through hipFree's own wait.
static int device_stage_reserve(dsdtm_localmap_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->d_cap) return DSDTM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    return ensure_stage(ctx, 0, std::max(bytes, (size_t)1 << 20));
}

// Room for `points` / `kfs` / `slots` elements in the map's arrays. An array that is too small is replaced by one of twice the
// size (at least the initial size and what is asked for, at most the limit), filled by a device-to-device copy on the stream; the
// old one is retired. All or nothing: when an allocation or a copy fails, the map keeps the arrays it had.
static int grow(dsdtm_localmap_ctx* ctx, dsdtm_localmap* m, int64_t points, int64_t kfs, int64_t slots) {
    struct Array { void** arr; int64_t* cap; int64_t used, need, initial, limit; size_t elem; void* fresh; int64_t fresh_cap; };
    Array arrays[3] = {
        {(void**)&m->d_points, &m->cap_points, m->n_points, points, LM_INITIAL_POINTS, DSDTM_LOCALMAP_MAX_POINTS, sizeof(LmPointDev), nullptr, 0},
        {(void**)&m->d_kfs, &m->cap_kfs, m->n_kfs, kfs, LM_INITIAL_KEYFRAMES, DSDTM_LOCALMAP_MAX_KEYFRAMES, sizeof(LmKeyframeDev), nullptr, 0},
        {(void**)&m->d_slots, &m->cap_slots, m->n_slots, slots, LM_INITIAL_SLOTS, (int64_t)DSDTM_LOCALMAP_MAX_KEYFRAMES * DSDTM_LOCALMAP_MAX_SLOTS,
         sizeof(int32_t), nullptr, 0}};
    auto drop = [&]() { for (Array& a : arrays) if (a.fresh) { (void)hipFree(a.fresh); a.fresh = nullptr; } };
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (Array& a : arrays) {
        if (a.need <= *a.cap) continue;
        a.fresh_cap = std::min(a.limit, std::max({a.need, a.initial, 2 * *a.cap}));
        hipError_t e = hipMalloc(&a.fresh, (size_t)a.fresh_cap * a.elem);
        if (e != hipSuccess) {
            a.fresh = nullptr;
            drop();
            set_err(ctx, "hipMalloc of %zu bytes for a map array failed: %s", (size_t)a.fresh_cap * a.elem, hipGetErrorString(e));
            return DSDTM_ERR_HIP;
        }
    }
    for (Array& a : arrays) {
        if (!a.fresh || a.used == 0) continue;
        hipError_t e = hipMemcpyAsync(a.fresh, *a.arr, (size_t)a.used * a.elem, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            set_err(ctx, "hipMemcpyAsync (a map array into its larger one) failed: %s", hipGetErrorString(e));
            (void)hipStreamSynchronize(ctx->stream);        // (a copy enqueued before this one writes into an array dropped here)
            drop();
            return DSDTM_ERR_HIP;
        }
    }
    for (Array& a : arrays) {
        if (!a.fresh) continue;
        if (*a.arr) ctx->retired.push_back(*a.arr);
        *a.arr = a.fresh;
        *a.cap = a.fresh_cap;
    }
    return DSDTM_OK;
}

// The staged bytes [h, h + bytes) to the device staging block (device_stage_reserve made the room), then ONE launch that copies its runs into the map's arrays
// (`src` of `a`: byte offsets into the staging block, as pointers from NULL).
static int apply(dsdtm_localmap_ctx* ctx, const uint8_t* h, size_t bytes, LmApplyArgs a) {
    for (int i = 0; i < 2; ++i) a.src[i] = (const uint32_t*)((const uint8_t*)ctx->d_stage + (size_t)(uintptr_t)a.src[i]);
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(localmap_apply_launch(a, ctx->stream));
    return DSDTM_OK;
}

extern "C" int dsdtm_localmap_points_write(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, int first, int n, const double* p_world, const uint8_t* bad) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "points_write: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || first < 0) { set_err(ctx, "points_write: %s is negative", n < 0 ? "n" : "first"); return DSDTM_ERR_INVALID; }
    if ((int64_t)first > map->n_points) { set_err(ctx, "points_write: first = %d leaves a gap behind the map's %lld points", first, (long long)map->n_points); return DSDTM_ERR_INVALID; }
    if ((int64_t)first + n > DSDTM_LOCALMAP_MAX_POINTS) { set_err(ctx, "points_write: first + n = %lld exceeds %d points", (long long)first + n, DSDTM_LOCALMAP_MAX_POINTS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!p_world) { set_err(ctx, "points_write: p_world is NULL"); return DSDTM_ERR_INVALID; }
    if (!all_finite(p_world, 3 * (size_t)n)) { set_err(ctx, "points_write: p_world is not finite"); return DSDTM_ERR_INVALID; }
    const int64_t end = (int64_t)first + n;
    uint8_t* h = nullptr;
    const size_t bytes = (size_t)n * sizeof(LmPointDev);
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (int rc = grow(ctx, map, end, 0, 0)) return rc;
    LmPointDev* rec = (LmPointDev*)h;
    for (int i = 0; i < n; ++i) {
        rec[i].x = p_world[3 * (size_t)i]; rec[i].y = p_world[3 * (size_t)i + 1]; rec[i].z = p_world[3 * (size_t)i + 2];
        rec[i].bad = bad && bad[i] ? 1u : 0u;
    }
    LmApplyArgs a{};
    a.dst[0] = (uint32_t*)(map->d_points + first); a.src[0] = nullptr; a.words[0] = (uint32_t)(bytes / 4);
    if (int rc = apply(ctx, h, bytes, a)) return rc;
    map->n_points = std::max(map->n_points, end);
    return DSDTM_OK;
}

// a slot is -1 (NULL) or a point the map has
static int bad_slot(const dsdtm_localmap* map, const int32_t* s, int n) {
    for (int i = 0; i < n; ++i) if (s[i] < -1 || (int64_t)s[i] >= map->n_points) return i;
    return -1;
}

extern "C" int dsdtm_localmap_keyframe_add(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                                           int* out_index) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "keyframe_add: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (!T_kf_w) { set_err(ctx, "keyframe_add: T_kf_w is NULL"); return DSDTM_ERR_INVALID; }
    if (n_slots < 0 || n_slots > DSDTM_LOCALMAP_MAX_SLOTS) { set_err(ctx, "keyframe_add: n_slots = %d outside 0..%d", n_slots, DSDTM_LOCALMAP_MAX_SLOTS); return DSDTM_ERR_INVALID; }
    if (n_slots > 0 && !point_of_slot) { set_err(ctx, "keyframe_add: point_of_slot is NULL"); return DSDTM_ERR_INVALID; }
    if (map->n_kfs >= DSDTM_LOCALMAP_MAX_KEYFRAMES) { set_err(ctx, "keyframe_add: the map holds %d keyframes already", DSDTM_LOCALMAP_MAX_KEYFRAMES); return DSDTM_ERR_INVALID; }
    if (!all_finite(T_kf_w, 12)) { set_err(ctx, "keyframe_add: T_kf_w is not finite"); return DSDTM_ERR_INVALID; }
    if (int i = bad_slot(map, point_of_slot, n_slots); i >= 0) {
        set_err(ctx, "keyframe_add: point_of_slot[%d] = %d is neither -1 nor below the map's %lld points", i, point_of_slot[i], (long long)map->n_points);
        return DSDTM_ERR_INVALID;
    }
    const size_t slot_bytes = (size_t)n_slots * 4, bytes = sizeof(LmKeyframeDev) + slot_bytes;
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (int rc = grow(ctx, map, 0, map->n_kfs + 1, map->n_slots + n_slots)) return rc;
    LmKeyframeDev rec;
    memset(&rec, 0, sizeof rec);
    memcpy(rec.T, T_kf_w, 96);
    rec.slot_off = map->n_slots; rec.n_slots = n_slots;
    memcpy(h, &rec, sizeof rec);
    if (n_slots) memcpy(h + sizeof rec, point_of_slot, slot_bytes);
    LmApplyArgs a{};
    a.dst[0] = (uint32_t*)(map->d_kfs + map->n_kfs); a.src[0] = nullptr; a.words[0] = (uint32_t)(sizeof rec / 4);
    a.dst[1] = (uint32_t*)(map->d_slots + map->n_slots); a.src[1] = (const uint32_t*)(uintptr_t)sizeof rec; a.words[1] = (uint32_t)n_slots;
    if (int rc = apply(ctx, h, bytes, a)) return rc;
    map->kf_n_slots.push_back(n_slots);
    map->kf_slot_off.push_back(map->n_slots);
    if (out_index) *out_index = (int)map->n_kfs;
    map->n_kfs += 1;
    map->n_slots += n_slots;
    return DSDTM_OK;
}

extern "C" int dsdtm_localmap_keyframe_write(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                                             const int32_t* point_of_slot) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "keyframe_write: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (kf < 0 || (int64_t)kf >= map->n_kfs) { set_err(ctx, "keyframe_write: keyframe %d: the map has %lld keyframes", kf, (long long)map->n_kfs); return DSDTM_ERR_INVALID; }
    const int have = map->kf_n_slots[(size_t)kf];
    if (n < 0 || first_slot < 0 || (int64_t)first_slot + n > have) {
        set_err(ctx, "keyframe_write: keyframe %d: slots [%d, %lld) outside its %d slots", kf, first_slot, (long long)first_slot + n, have);
        return DSDTM_ERR_INVALID;
    }
    if (n > 0 && !point_of_slot) { set_err(ctx, "keyframe_write: keyframe %d: point_of_slot is NULL", kf); return DSDTM_ERR_INVALID; }
    if (T_kf_w && !all_finite(T_kf_w, 12)) { set_err(ctx, "keyframe_write: keyframe %d: T_kf_w is not finite", kf); return DSDTM_ERR_INVALID; }
    if (int i = bad_slot(map, point_of_slot, n); i >= 0) {
        set_err(ctx, "keyframe_write: keyframe %d: point_of_slot[%d] = %d is neither -1 nor below the map's %lld points", kf, i, point_of_slot[i],
                (long long)map->n_points);
        return DSDTM_ERR_INVALID;
    }
    if (!T_kf_w && n == 0) return DSDTM_OK;
    const size_t pose_bytes = T_kf_w ? 96 : 0, bytes = pose_bytes + (size_t)n * 4;
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (T_kf_w) memcpy(h, T_kf_w, 96);
    if (n) memcpy(h + pose_bytes, point_of_slot, (size_t)n * 4);
    LmApplyArgs a{};
    a.dst[0] = (uint32_t*)map->d_kfs[kf].T; a.src[0] = nullptr; a.words[0] = (uint32_t)(pose_bytes / 4);
    a.dst[1] = (uint32_t*)(map->d_slots + map->kf_slot_off[(size_t)kf] + first_slot); a.src[1] = (const uint32_t*)(uintptr_t)pose_bytes; a.words[1] = (uint32_t)n;
    return apply(ctx, h, bytes, a);
}

extern "C" int dsdtm_localmap_map_read(dsdtm_localmap_ctx* ctx, const dsdtm_localmap* map, dsdtm_localmap_image* out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "map_read: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (!out) { set_err(ctx, "map_read: out is NULL"); return DSDTM_ERR_INVALID; }
    const size_t P = (size_t)map->n_points, K = (size_t)map->n_kfs, S = (size_t)map->n_slots;
    const bool fits = out->point_capacity >= 0 && (size_t)out->point_capacity >= P && out->keyframe_capacity >= 0 && (size_t)out->keyframe_capacity >= K &&
                      out->slot_capacity >= 0 && (size_t)out->slot_capacity >= S;
    if (fits) {
        const char* missing = P && !out->p_world ? "p_world" : P && !out->bad ? "bad" : K && !out->T_kf_w ? "T_kf_w" : K && !out->n_slots ? "n_slots"
                            : K && !out->slot_offset ? "slot_offset" : S && !out->point_of_slot ? "point_of_slot" : nullptr;
        if (missing) { set_err(ctx, "map_read: %s is NULL", missing); return DSDTM_ERR_INVALID; }
        // (pageable destinations: the call is synchronous, and a checkpoint is no per-frame path)
        std::vector<LmPointDev> pts(P);
        std::vector<LmKeyframeDev> kfs(K);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
        if (P) API_TRY(hipMemcpyAsync(pts.data(), map->d_points, P * sizeof(LmPointDev), hipMemcpyDeviceToHost, ctx->stream));
        if (K) API_TRY(hipMemcpyAsync(kfs.data(), map->d_kfs, K * sizeof(LmKeyframeDev), hipMemcpyDeviceToHost, ctx->stream));
        if (S) API_TRY(hipMemcpyAsync(out->point_of_slot, map->d_slots, S * 4, hipMemcpyDeviceToHost, ctx->stream));
        API_TRY(hipStreamSynchronize(ctx->stream));
        stream_idle(ctx);
        for (size_t i = 0; i < P; ++i) {
            out->p_world[3 * i] = pts[i].x; out->p_world[3 * i + 1] = pts[i].y; out->p_world[3 * i + 2] = pts[i].z;
            out->bad[i] = pts[i].bad ? 1 : 0;
        }
        for (size_t k = 0; k < K; ++k) {
            memcpy(out->T_kf_w + 12 * k, kfs[k].T, 96);
            out->n_slots[k] = kfs[k].n_slots; out->slot_offset[k] = kfs[k].slot_off;
        }
    }
    out->n_points = (int32_t)P; out->n_keyframes = (int32_t)K; out->n_slots_total = (int64_t)S;
    out->complete = fits ? 1 : 0; out->reserved = 0;
    return DSDTM_OK;
}

// One upload (the descs: poses, the maps' arrays, the offsets of keys and outputs in the device block), two launches, one read-back of
// every desc's outputs, one wait.
extern "C" int dsdtm_localmap_select(dsdtm_localmap_ctx* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                                     const dsdtm_localmap_desc* descs, dsdtm_localmap_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam) { set_err(ctx, "select: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!prm) { set_err(ctx, "select: params is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_LOCALMAP_MAX_DESCS) { set_err(ctx, "select: n = %d outside 0..%d", n, DSDTM_LOCALMAP_MAX_DESCS); return DSDTM_ERR_INVALID; }
    if (prm->n_local < 1 || prm->n_local > DSDTM_LOCALMAP_MAX_LOCAL) { set_err(ctx, "select: n_local = %d outside 1..%d", prm->n_local, DSDTM_LOCALMAP_MAX_LOCAL); return DSDTM_ERR_INVALID; }
    if (prm->boundary < 0) { set_err(ctx, "select: boundary = %d is negative", prm->boundary); return DSDTM_ERR_INVALID; }
    if (cam->width <= 0 || cam->height <= 0) { set_err(ctx, "select: camera size %d x %d is not positive", cam->width, cam->height); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs || !results) { set_err(ctx, "select: %s is NULL", !descs ? "descs" : "results"); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the block's layout on the way: descs | outputs | keys
    const size_t N = (size_t)n, L = (size_t)prm->n_local;
    std::vector<LmDescDev> rec(N);
    size_t o = align_up(N * sizeof(LmDescDev), 16);
    int max_K = 0, max_P = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_localmap_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (!owns(ctx, d.map)) bad = "map is not a map of this context";
        else if (!d.T_cur_w) bad = "T_cur_w is NULL";
        else if (!d.kf) bad = "kf is NULL";
        else if (!d.kf_dist) bad = "kf_dist is NULL";
        else if (d.point_capacity < 0 || (int64_t)d.point_capacity > (int64_t)prm->n_local * DSDTM_LOCALMAP_MAX_SLOTS) bad = "point_capacity out of range";
        else if (d.point_capacity > 0 && !d.point) bad = "point is NULL";
        else if (d.point_capacity > 0 && !d.point_kf) bad = "point_kf is NULL";
        else if (!all_finite(d.T_cur_w, 12)) bad = "T_cur_w is not finite";
        if (bad) { set_err(ctx, "select: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        LmDescDev& r = rec[(size_t)t];
        memset(&r, 0, sizeof r);
        memcpy(r.T, d.T_cur_w, 96);
        r.points = d.map->d_points; r.kfs = d.map->d_kfs; r.slots = d.map->d_slots;
        r.K = (int32_t)d.map->n_kfs; r.P = (int32_t)d.map->n_points; r.capacity = d.point_capacity;
        max_K = std::max(max_K, r.K); max_P = std::max(max_P, r.P);
        const size_t cap = (size_t)d.point_capacity;
        r.kf_dist = o; o += L * 8;
        r.result = o; o += sizeof(dsdtm_localmap_result);
        r.kf = o; o += L * 4;
        r.point = o; o += cap * 4;
        r.point_kf = o; o += cap * 4;
        o = align_up(o, 8);
    }
    const size_t back = align_up(o, 256);       // what comes back: everything in front of the keys
    o = back;
    for (int t = 0; t < n; ++t) { rec[(size_t)t].keys = o; o += (size_t)rec[(size_t)t].K * 8; }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, std::max(o, back))) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    const size_t up = N * sizeof(LmDescDev), out0 = align_up(up, 16);
    memcpy(h, rec.data(), up);
    LmSelectArgs a;
    memset(&a, 0, sizeof a);
    a.block = g; a.n = n; a.max_K = max_K; a.max_P = max_P; a.n_local = prm->n_local; a.boundary = prm->boundary;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.width = cam->width; a.height = cam->height;
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(localmap_select_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + out0, g + out0, back - out0, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    for (int t = 0; t < n; ++t) {
        const dsdtm_localmap_desc& d = descs[t];
        const LmDescDev& r = rec[(size_t)t];
        dsdtm_localmap_result res;
        memcpy(&res, h + r.result, sizeof res);
        const size_t n_kf = (size_t)std::min(std::max(res.n_kf, 0), prm->n_local);
        const size_t n_pt = (size_t)std::min(std::max(res.n_points, 0), d.point_capacity);
        if (n_kf) { memcpy(d.kf, h + r.kf, n_kf * 4); memcpy(d.kf_dist, h + r.kf_dist, n_kf * 8); }
        if (n_pt) { memcpy(d.point, h + r.point, n_pt * 4); memcpy(d.point_kf, h + r.point_kf, n_pt * 4); }
        results[t] = res;
    }
    return DSDTM_OK;
}
