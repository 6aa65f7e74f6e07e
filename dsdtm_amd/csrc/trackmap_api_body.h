// trackmap_api_body.h — the C ABI of include/dsdtm_amd_trackmap.h: the resident track map, its updates, the checks and the packing of a
// dsdtm_trackmap_local call (the context: addon_host.h). ONE implementation, compiled once per library that serves the map: the
// including translation unit names the entries (TM_API(local) -> dsdtm_trackmap_local in trackmap_api.cpp, dsdtm_mapping_local in
// mapping_api.cpp), the context type (TM_CTX) and the library as its messages call it (TM_LIB) before it includes this file.
//
// A map is six device arrays in three groups that grow together — per point the LmPointDev record and the found count; the keyframe
// records; per slot of the pool point_of_slot, the observing point (the point index when the slot observes, -1 otherwise: what the
// flatten scans) and the feature record — and, on the host, only what the checks need: the counts and each keyframe's slot count and
// offset. An UPDATE is staged in the context's pinned block — handed out piece by piece, so that an update never overwrites what an
// earlier one has staged and the stream has not yet read — then moved by one copy into the device staging block and applied by
// ONE launch: an update that fails at any HIP call has changed nothing. A LOCAL call is one upload (both desc arrays), the two
// launches of localmap.hip, the launches of trackmap.hip, one read-back of every desc's outputs and one wait. There is no CPU compute
// path here (the host evaluation is host/dsdtm_trackmap_host.hpp, which needs no library).
#if !defined(TM_API) || !defined(TM_CTX) || !defined(TM_LIB)
#error "trackmap_api_body.h: define TM_API(name), TM_CTX and TM_LIB before including it (see trackmap_api.cpp)"
#endif
#ifdef DSDTM_TRACKMAP_API_BODY_H
#error "trackmap_api_body.h defines the entries of ONE library: include it once per translation unit"
#endif
#define DSDTM_TRACKMAP_API_BODY_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "trackmap.h"
#include "addon_host.h"

using namespace dsdtm;

struct dsdtm_trackmap {
    LmPointDev* d_points = nullptr; int32_t* d_found = nullptr;                             // group 0: per point
    LmKeyframeDev* d_kfs = nullptr;                                                         // group 1: per keyframe
    int32_t* d_slots = nullptr; int32_t* d_obs = nullptr; TmFeatDev* d_feat = nullptr;      // group 2: per slot of the pool
    int64_t cap[3] = {0, 0, 0};         // elements allocated per group
    int64_t used[3] = {0, 0, 0};        // points, keyframes, slots in use, as of the last update enqueued
    std::vector<int32_t> kf_n_slots;    // per keyframe: what keyframe_write and map_read check against
    std::vector<int64_t> kf_slot_off;
};

struct TM_CTX : dsdtm::AddonCtx {
    std::vector<dsdtm_trackmap*> maps;
    std::vector<void*> retired;     // device arrays a map has outgrown: freed once the stream has been waited for
    size_t h_used = 0;              // bytes of the pinned block handed out since the stream was last waited for
};

static void release_retired(TM_CTX* ctx) {
    for (void* p : ctx->retired) (void)hipFree(p);
    ctx->retired.clear();
}

// the stream has run dry: every staged byte has been read, every outgrown array has been passed
static void stream_idle(TM_CTX* ctx) {
    ctx->h_used = 0;
    release_retired(ctx);
}

static void free_map(dsdtm_trackmap* m) {
    void* arrays[6] = {m->d_points, m->d_found, m->d_kfs, m->d_slots, m->d_obs, m->d_feat};
    for (void* p : arrays) if (p) (void)hipFree(p);
    delete m;
}

extern "C" const char* TM_API(last_error)(const TM_CTX* ctx) { return addon_last_error(ctx); }
extern "C" int TM_API(create)(int device, TM_CTX** out) { return addon_create(TM_LIB, device, out); }
extern "C" void TM_API(destroy)(TM_CTX* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (dsdtm_trackmap* m : ctx->maps) free_map(m);
    ctx->maps.clear();
    release_retired(ctx);
    addon_destroy(ctx);
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

static bool owns(const TM_CTX* ctx, const dsdtm_trackmap* map) {
    return map && std::find(ctx->maps.begin(), ctx->maps.end(), map) != ctx->maps.end();
}

extern "C" int TM_API(map_create)(TM_CTX* ctx, dsdtm_trackmap** out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!out) { set_err(ctx, "map_create: out is NULL"); return DSDTM_ERR_INVALID; }
    *out = nullptr;
    dsdtm_trackmap* m = new (std::nothrow) dsdtm_trackmap();
    if (!m) { set_err(ctx, "map_create: out of host memory"); return DSDTM_ERR_NOMEM; }
    ctx->maps.push_back(m);         // (the device arrays come with the first update that needs them)
    *out = m;
    return DSDTM_OK;
}

extern "C" void TM_API(map_destroy)(TM_CTX* ctx, dsdtm_trackmap* map) {
    if (!ctx || !owns(ctx, map)) return;
    (void)hipSetDevice(ctx->device);
    if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx);      // (updates of this map may still be on their way)
    ctx->maps.erase(std::find(ctx->maps.begin(), ctx->maps.end(), map));
    free_map(map);
}

// `bytes` of the pinned block that no earlier update still needs
static int pinned_reserve(TM_CTX* ctx, size_t bytes, uint8_t** out) {
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
static int device_stage_reserve(TM_CTX* ctx, size_t bytes) {
    if (bytes <= ctx->d_cap) return DSDTM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    return ensure_stage(ctx, 0, std::max(bytes, (size_t)1 << 20));
}

// Room for `points` / `kfs` / `slots` elements. A group that is too small gets arrays of twice the size (at least the initial size and
// what is asked for, at most the limit), filled by device-to-device copies on the stream; the old ones are retired. All or nothing:
// when an allocation or a copy fails, the map keeps the arrays it had.
static int grow(TM_CTX* ctx, dsdtm_trackmap* m, int64_t points, int64_t kfs, int64_t slots) {
    struct Array { void** arr; int group; size_t elem; void* fresh; };
    Array arrays[6] = {{(void**)&m->d_points, 0, sizeof(LmPointDev), nullptr}, {(void**)&m->d_found, 0, sizeof(int32_t), nullptr},
                       {(void**)&m->d_kfs, 1, sizeof(LmKeyframeDev), nullptr},
                       {(void**)&m->d_slots, 2, sizeof(int32_t), nullptr}, {(void**)&m->d_obs, 2, sizeof(int32_t), nullptr},
                       {(void**)&m->d_feat, 2, sizeof(TmFeatDev), nullptr}};
    const int64_t need[3] = {points, kfs, slots};
    const int64_t initial[3] = {LM_INITIAL_POINTS, LM_INITIAL_KEYFRAMES, LM_INITIAL_SLOTS};
    const int64_t limit[3] = {DSDTM_LOCALMAP_MAX_POINTS, DSDTM_LOCALMAP_MAX_KEYFRAMES, (int64_t)DSDTM_LOCALMAP_MAX_KEYFRAMES * DSDTM_LOCALMAP_MAX_SLOTS};
    int64_t fresh_cap[3] = {0, 0, 0};
    for (int g = 0; g < 3; ++g)
        if (need[g] > m->cap[g]) fresh_cap[g] = std::min(limit[g], std::max({need[g], initial[g], 2 * m->cap[g]}));
    auto drop = [&]() { for (Array& a : arrays) if (a.fresh) { (void)hipFree(a.fresh); a.fresh = nullptr; } };
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (Array& a : arrays) {
        if (!fresh_cap[a.group]) continue;
        hipError_t e = hipMalloc(&a.fresh, (size_t)fresh_cap[a.group] * a.elem);
        if (e != hipSuccess) {
            a.fresh = nullptr;
            drop();
            set_err(ctx, "hipMalloc of %zu bytes for a map array failed: %s", (size_t)fresh_cap[a.group] * a.elem, hipGetErrorString(e));
            return DSDTM_ERR_HIP;
        }
    }
    for (Array& a : arrays) {
        if (!a.fresh || m->used[a.group] == 0) continue;
        hipError_t e = hipMemcpyAsync(a.fresh, *a.arr, (size_t)m->used[a.group] * a.elem, hipMemcpyDeviceToDevice, ctx->stream);
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
    }
    for (int g = 0; g < 3; ++g) if (fresh_cap[g]) m->cap[g] = fresh_cap[g];
    return DSDTM_OK;
}

// The staged bytes [h, h + bytes) to the device staging block (device_stage_reserve made the room). The launch that applies them
// follows on the same stream.
static int upload_staged(TM_CTX* ctx, const uint8_t* h, size_t bytes) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return DSDTM_OK;
}

extern "C" int TM_API(points_write)(TM_CTX* ctx, dsdtm_trackmap* map, int first, int n, const double* p_world, const uint8_t* bad,
                                           const int32_t* found) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "points_write: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || first < 0) { set_err(ctx, "points_write: %s is negative", n < 0 ? "n" : "first"); return DSDTM_ERR_INVALID; }
    if ((int64_t)first > map->used[0]) { set_err(ctx, "points_write: first = %d leaves a gap behind the map's %lld points", first, (long long)map->used[0]); return DSDTM_ERR_INVALID; }
    if ((int64_t)first + n > DSDTM_LOCALMAP_MAX_POINTS) { set_err(ctx, "points_write: first + n = %lld exceeds %d points", (long long)first + n, DSDTM_LOCALMAP_MAX_POINTS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!p_world) { set_err(ctx, "points_write: p_world is NULL"); return DSDTM_ERR_INVALID; }
    if (!all_finite(p_world, 3 * (size_t)n)) { set_err(ctx, "points_write: p_world is not finite"); return DSDTM_ERR_INVALID; }
    const int64_t end = (int64_t)first + n;
    const size_t N = (size_t)n, o_found = N * 24, o_bad = o_found + (found ? N * 4 : 0), bytes = o_bad + (bad ? N : 0);     // xyz | found | bad
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (int rc = grow(ctx, map, end, 0, 0)) return rc;
    memcpy(h, p_world, N * 24);
    if (found) memcpy(h + o_found, found, N * 4);
    if (bad) memcpy(h + o_bad, bad, N);
    const uint8_t* g = (const uint8_t*)ctx->d_stage;
    TmPointsArgs a;
    memset(&a, 0, sizeof a);
    a.points = map->d_points; a.found_dst = map->d_found; a.xyz = (const double*)g;
    a.found = found ? (const int32_t*)(g + o_found) : nullptr; a.bad = bad ? g + o_bad : nullptr;
    a.first = first; a.n = n; a.old_count = (int32_t)map->used[0];
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    if (int rc = upload_staged(ctx, h, bytes)) return rc;
    API_TRY(trackmap_points_launch(a, ctx->stream));
    map->used[0] = std::max(map->used[0], end);
    return DSDTM_OK;
}

extern "C" int TM_API(found_write)(TM_CTX* ctx, dsdtm_trackmap* map, int n, const int32_t* index, const int32_t* found) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "found_write: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0) { set_err(ctx, "found_write: n is negative"); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!index || !found) { set_err(ctx, "found_write: %s is NULL", !index ? "index" : "found"); return DSDTM_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (index[i] < 0 || (int64_t)index[i] >= map->used[0]) {
            set_err(ctx, "found_write: index[%d] = %d is not below the map's %lld points", i, index[i], (long long)map->used[0]);
            return DSDTM_ERR_INVALID;
        }
    std::vector<int32_t> sorted(index, index + n);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    if (dup != sorted.end()) { set_err(ctx, "found_write: index %d occurs twice", *dup); return DSDTM_ERR_INVALID; }
    const size_t N = (size_t)n, bytes = N * 8;
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    memcpy(h, index, N * 4);
    memcpy(h + N * 4, found, N * 4);
    const int32_t* g = (const int32_t*)ctx->d_stage;
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    if (int rc = upload_staged(ctx, h, bytes)) return rc;
    API_TRY(trackmap_found_launch(map->d_found, g, g + N, n, ctx->stream));
    return DSDTM_OK;
}

// a slot is -1 (NULL) or a point the map has; its flag is 0 or 1, and 1 only on a point. Returns the message's tail, or NULL.
static const char* bad_slot(const dsdtm_trackmap* map, const int32_t* s, const uint8_t* obs, int n, int* at) {
    for (int i = 0; i < n; ++i) {
        *at = i;
        if (s[i] < -1 || (int64_t)s[i] >= map->used[0]) return "point_of_slot[%d] = %d is neither -1 nor below the map's %lld points";
        if (obs[i] > 1) return "observes[%d] is neither 0 nor 1 (point_of_slot %d; the map has %lld points)";
        if (obs[i] == 1 && s[i] < 0) return "observes[%d] = 1 on a NULL slot (point_of_slot %d; the map has %lld points)";
    }
    return nullptr;
}

// the observing point of each slot: what the flatten scans
static void observing(int32_t* dst, const int32_t* s, const uint8_t* obs, int n) {
    for (int i = 0; i < n; ++i) dst[i] = obs[i] ? s[i] : -1;
}

extern "C" int TM_API(keyframe_add)(TM_CTX* ctx, dsdtm_trackmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                                           const uint8_t* observes, const float* px_xy, const int32_t* level, const double* bearing, int* out_index) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "keyframe_add: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (!T_kf_w) { set_err(ctx, "keyframe_add: T_kf_w is NULL"); return DSDTM_ERR_INVALID; }
    if (n_slots < 0 || n_slots > DSDTM_LOCALMAP_MAX_SLOTS) { set_err(ctx, "keyframe_add: n_slots = %d outside 0..%d", n_slots, DSDTM_LOCALMAP_MAX_SLOTS); return DSDTM_ERR_INVALID; }
    if (n_slots > 0) {
        const char* missing = !point_of_slot ? "point_of_slot" : !observes ? "observes" : !px_xy ? "px_xy" : !level ? "level" : !bearing ? "bearing" : nullptr;
        if (missing) { set_err(ctx, "keyframe_add: %s is NULL", missing); return DSDTM_ERR_INVALID; }
    }
    if (map->used[1] >= DSDTM_LOCALMAP_MAX_KEYFRAMES) { set_err(ctx, "keyframe_add: the map holds %d keyframes already", DSDTM_LOCALMAP_MAX_KEYFRAMES); return DSDTM_ERR_INVALID; }
    if (!all_finite(T_kf_w, 12)) { set_err(ctx, "keyframe_add: T_kf_w is not finite"); return DSDTM_ERR_INVALID; }
    int at = 0;
    if (const char* why = bad_slot(map, point_of_slot, observes, n_slots, &at)) {
        char fmt[256];
        snprintf(fmt, sizeof fmt, "keyframe_add: %s", why);
        set_err(ctx, fmt, at, point_of_slot[at], (long long)map->used[0]);
        return DSDTM_ERR_INVALID;
    }
    const size_t S = (size_t)n_slots, o_slots = sizeof(LmKeyframeDev), o_obs = o_slots + S * 4, o_feat = align_up(o_obs + S * 4, 8),
                 bytes = o_feat + S * sizeof(TmFeatDev);
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (int rc = grow(ctx, map, 0, map->used[1] + 1, map->used[2] + n_slots)) return rc;
    LmKeyframeDev rec;
    memset(&rec, 0, sizeof rec);
    memcpy(rec.T, T_kf_w, 96);
    rec.slot_off = map->used[2]; rec.n_slots = n_slots;
    memset(h, 0, bytes);
    memcpy(h, &rec, sizeof rec);
    if (n_slots) {
        memcpy(h + o_slots, point_of_slot, S * 4);
        observing((int32_t*)(h + o_obs), point_of_slot, observes, n_slots);
        TmFeatDev* f = (TmFeatDev*)(h + o_feat);
        for (size_t s = 0; s < S; ++s) {
            f[s].px[0] = px_xy[2 * s]; f[s].px[1] = px_xy[2 * s + 1]; f[s].level = level[s];
            memcpy(f[s].bearing, bearing + 3 * s, 24);
        }
    }
    const uint8_t* g = (const uint8_t*)ctx->d_stage;
    TmApplyArgs a{};
    a.dst[0] = (uint32_t*)(map->d_kfs + map->used[1]); a.src[0] = (const uint32_t*)g; a.words[0] = (uint32_t)(sizeof rec / 4);
    a.dst[1] = (uint32_t*)(map->d_slots + map->used[2]); a.src[1] = (const uint32_t*)(g + o_slots); a.words[1] = (uint32_t)S;
    a.dst[2] = (uint32_t*)(map->d_obs + map->used[2]); a.src[2] = (const uint32_t*)(g + o_obs); a.words[2] = (uint32_t)S;
    a.dst[3] = (uint32_t*)(map->d_feat + map->used[2]); a.src[3] = (const uint32_t*)(g + o_feat); a.words[3] = (uint32_t)(S * sizeof(TmFeatDev) / 4);
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    if (int rc = upload_staged(ctx, h, bytes)) return rc;
    API_TRY(trackmap_apply_launch(a, ctx->stream));
    map->kf_n_slots.push_back(n_slots);
    map->kf_slot_off.push_back(map->used[2]);
    if (out_index) *out_index = (int)map->used[1];
    map->used[1] += 1;
    map->used[2] += n_slots;
    return DSDTM_OK;
}

extern "C" int TM_API(keyframe_write)(TM_CTX* ctx, dsdtm_trackmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                                             const int32_t* point_of_slot, const uint8_t* observes) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "keyframe_write: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (kf < 0 || (int64_t)kf >= map->used[1]) { set_err(ctx, "keyframe_write: keyframe %d: the map has %lld keyframes", kf, (long long)map->used[1]); return DSDTM_ERR_INVALID; }
    const int have = map->kf_n_slots[(size_t)kf];
    if (n < 0 || first_slot < 0 || (int64_t)first_slot + n > have) {
        set_err(ctx, "keyframe_write: keyframe %d: slots [%d, %lld) outside its %d slots", kf, first_slot, (long long)first_slot + n, have);
        return DSDTM_ERR_INVALID;
    }
    if (n > 0 && (!point_of_slot || !observes)) { set_err(ctx, "keyframe_write: keyframe %d: %s is NULL", kf, !point_of_slot ? "point_of_slot" : "observes"); return DSDTM_ERR_INVALID; }
    if (T_kf_w && !all_finite(T_kf_w, 12)) { set_err(ctx, "keyframe_write: keyframe %d: T_kf_w is not finite", kf); return DSDTM_ERR_INVALID; }
    int at = 0;
    if (const char* why = bad_slot(map, point_of_slot, observes, n, &at)) {
        char fmt[256];
        snprintf(fmt, sizeof fmt, "keyframe_write: keyframe %d: %s", kf, why);
        set_err(ctx, fmt, at, point_of_slot[at], (long long)map->used[0]);
        return DSDTM_ERR_INVALID;
    }
    if (!T_kf_w && n == 0) return DSDTM_OK;
    const size_t S = (size_t)n, pose_bytes = T_kf_w ? 96 : 0, o_obs = pose_bytes + S * 4, bytes = o_obs + S * 4;
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, bytes)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, bytes, &h)) return rc;
    if (T_kf_w) memcpy(h, T_kf_w, 96);
    if (n) {
        memcpy(h + pose_bytes, point_of_slot, S * 4);
        observing((int32_t*)(h + o_obs), point_of_slot, observes, n);
    }
    const uint8_t* g = (const uint8_t*)ctx->d_stage;
    const int64_t at_slot = map->kf_slot_off[(size_t)kf] + first_slot;
    TmApplyArgs a{};
    a.dst[0] = (uint32_t*)map->d_kfs[kf].T; a.src[0] = (const uint32_t*)g; a.words[0] = (uint32_t)(pose_bytes / 4);
    a.dst[1] = (uint32_t*)(map->d_slots + at_slot); a.src[1] = (const uint32_t*)(g + pose_bytes); a.words[1] = (uint32_t)S;
    a.dst[2] = (uint32_t*)(map->d_obs + at_slot); a.src[2] = (const uint32_t*)(g + o_obs); a.words[2] = (uint32_t)S;
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    if (int rc = upload_staged(ctx, h, bytes)) return rc;
    API_TRY(trackmap_apply_launch(a, ctx->stream));
    return DSDTM_OK;
}

extern "C" int TM_API(map_read)(TM_CTX* ctx, const dsdtm_trackmap* map, dsdtm_trackmap_image* out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!owns(ctx, map)) { set_err(ctx, "map_read: map is %s", map ? "not a map of this context" : "NULL"); return DSDTM_ERR_INVALID; }
    if (!out) { set_err(ctx, "map_read: out is NULL"); return DSDTM_ERR_INVALID; }
    const size_t P = (size_t)map->used[0], K = (size_t)map->used[1], S = (size_t)map->used[2];
    const bool fits = out->point_capacity >= 0 && (size_t)out->point_capacity >= P && out->keyframe_capacity >= 0 && (size_t)out->keyframe_capacity >= K &&
                      out->slot_capacity >= 0 && (size_t)out->slot_capacity >= S;
    if (fits) {
        const char* missing = P && !out->p_world ? "p_world" : P && !out->bad ? "bad" : P && !out->found ? "found" : K && !out->T_kf_w ? "T_kf_w"
                            : K && !out->n_slots ? "n_slots" : K && !out->slot_offset ? "slot_offset" : S && !out->point_of_slot ? "point_of_slot"
                            : S && !out->observes ? "observes" : S && !out->px_xy ? "px_xy" : S && !out->level ? "level" : S && !out->bearing ? "bearing" : nullptr;
        if (missing) { set_err(ctx, "map_read: %s is NULL", missing); return DSDTM_ERR_INVALID; }
        // (pageable destinations: the call is synchronous, and a checkpoint is no per-frame path)
        std::vector<LmPointDev> pts(P);
        std::vector<LmKeyframeDev> kfs(K);
        std::vector<int32_t> obs(S);
        std::vector<TmFeatDev> feat(S);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
        if (P) API_TRY(hipMemcpyAsync(pts.data(), map->d_points, P * sizeof(LmPointDev), hipMemcpyDeviceToHost, ctx->stream));
        if (P) API_TRY(hipMemcpyAsync(out->found, map->d_found, P * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (K) API_TRY(hipMemcpyAsync(kfs.data(), map->d_kfs, K * sizeof(LmKeyframeDev), hipMemcpyDeviceToHost, ctx->stream));
        if (S) API_TRY(hipMemcpyAsync(out->point_of_slot, map->d_slots, S * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (S) API_TRY(hipMemcpyAsync(obs.data(), map->d_obs, S * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (S) API_TRY(hipMemcpyAsync(feat.data(), map->d_feat, S * sizeof(TmFeatDev), hipMemcpyDeviceToHost, ctx->stream));
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
        for (size_t s = 0; s < S; ++s) {
            out->observes[s] = obs[s] >= 0 ? 1 : 0;
            out->px_xy[2 * s] = feat[s].px[0]; out->px_xy[2 * s + 1] = feat[s].px[1]; out->level[s] = feat[s].level;
            memcpy(out->bearing + 3 * s, feat[s].bearing, 24);
        }
    }
    out->n_points = (int32_t)P; out->n_keyframes = (int32_t)K; out->n_slots_total = (int64_t)S;
    out->complete = fits ? 1 : 0; out->reserved = 0;
    return DSDTM_OK;
}

// One upload (the two desc arrays: poses, the maps' arrays, the offsets of outputs and temporaries in the device block), the
// launches, one read-back of every desc's outputs, one wait.
extern "C" int TM_API(local)(TM_CTX* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                                    const dsdtm_trackmap_desc* descs, dsdtm_trackmap_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (!cam) { set_err(ctx, "local: cam is NULL"); return DSDTM_ERR_INVALID; }
    if (!prm) { set_err(ctx, "local: params is NULL"); return DSDTM_ERR_INVALID; }
    if (n < 0 || n > DSDTM_LOCALMAP_MAX_DESCS) { set_err(ctx, "local: n = %d outside 0..%d", n, DSDTM_LOCALMAP_MAX_DESCS); return DSDTM_ERR_INVALID; }
    if (prm->n_local < 1 || prm->n_local > DSDTM_LOCALMAP_MAX_LOCAL) { set_err(ctx, "local: n_local = %d outside 1..%d", prm->n_local, DSDTM_LOCALMAP_MAX_LOCAL); return DSDTM_ERR_INVALID; }
    if (prm->boundary < 0) { set_err(ctx, "local: boundary = %d is negative", prm->boundary); return DSDTM_ERR_INVALID; }
    if (cam->width <= 0 || cam->height <= 0) { set_err(ctx, "local: camera size %d x %d is not positive", cam->width, cam->height); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs || !results) { set_err(ctx, "local: %s is NULL", !descs ? "descs" : "results"); return DSDTM_ERR_INVALID; }
    // every desc is checked before anything is enqueued; the block's layout on the way: LmDescDev x n | TmDescDev x n | outputs | temporaries
    const size_t N = (size_t)n, L = (size_t)prm->n_local;
    std::vector<LmDescDev> lrec(N);
    std::vector<TmDescDev> trec(N);
    const size_t descs_off = align_up(N * sizeof(LmDescDev), 16), up = descs_off + N * sizeof(TmDescDev), out0 = align_up(up, 16);
    size_t o = out0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 8); return (uint64_t)at; };
    int max_K = 0, max_P = 0, max_cap = 0, max_ocap = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_trackmap_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (!owns(ctx, d.map)) bad = "map is not a map of this context";
        else if (!d.T_cur_w) bad = "T_cur_w is NULL";
        else if (!d.kf) bad = "kf is NULL";
        else if (!d.kf_dist) bad = "kf_dist is NULL";
        else if (d.point_capacity < 0 || d.point_capacity > DSDTM_TRACKMAP_MAX_LOCAL_POINTS) bad = "point_capacity out of range";
        else if (d.obs_capacity < 0) bad = "obs_capacity is negative";
        else if (!d.obs_offset) bad = "obs_offset is NULL";
        else if (d.point_capacity > 0 && !d.point) bad = "point is NULL";
        else if (d.point_capacity > 0 && !d.point_kf) bad = "point_kf is NULL";
        else if (d.point_capacity > 0 && !d.mp_world) bad = "mp_world is NULL";
        else if (d.point_capacity > 0 && !d.mp_found) bad = "mp_found is NULL";
        else if (d.point_capacity > 0 && !d.mp_bad) bad = "mp_bad is NULL";
        else if (d.obs_capacity > 0 && !d.obs_kf) bad = "obs_kf is NULL";
        else if (d.obs_capacity > 0 && !d.obs_px) bad = "obs_px is NULL";
        else if (d.obs_capacity > 0 && !d.obs_level) bad = "obs_level is NULL";
        else if (d.obs_capacity > 0 && !d.obs_bearing) bad = "obs_bearing is NULL";
        else if (!all_finite(d.T_cur_w, 12)) bad = "T_cur_w is not finite";
        if (bad) { set_err(ctx, "local: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        LmDescDev& r = lrec[(size_t)t];
        TmDescDev& q = trec[(size_t)t];
        memset(&r, 0, sizeof r);
        memset(&q, 0, sizeof q);
        memcpy(r.T, d.T_cur_w, 96);
        r.points = d.map->d_points; r.kfs = d.map->d_kfs; r.slots = d.map->d_slots;
        r.K = (int32_t)d.map->used[1]; r.P = (int32_t)d.map->used[0]; r.capacity = d.point_capacity;
        q.found = d.map->d_found; q.obs = d.map->d_obs; q.feat = d.map->d_feat; q.ocap = d.obs_capacity;
        max_K = std::max(max_K, r.K); max_P = std::max(max_P, r.P);
        max_cap = std::max(max_cap, d.point_capacity); max_ocap = std::max(max_ocap, d.obs_capacity);
        const size_t cap = (size_t)d.point_capacity, ocap = (size_t)d.obs_capacity;
        r.kf_dist = take(L * 8); r.result = take(sizeof(dsdtm_localmap_result)); q.ext = take(sizeof(TmExtResult));
        r.kf = take(L * 4); r.point = take(cap * 4); r.point_kf = take(cap * 4);
        q.mp_world = take(cap * 24); q.mp_found = take(cap * 4); q.mp_bad = take(cap); q.obs_offset = take((cap + 1) * 4);
        q.obs_kf = take(ocap * 4); q.obs_px = take(ocap * 8); q.obs_level = take(ocap * 4); q.obs_bearing = take(ocap * 24);
        if (o > (size_t)DSDTM_TRACKMAP_MAX_CALL_BYTES) break;      // (refused below; the sum cannot wrap)
    }
    const size_t back = align_up(o, 256);       // what comes back: everything in front of the temporaries
    o = back;
    for (int t = 0; t < n && o <= (size_t)DSDTM_TRACKMAP_MAX_CALL_BYTES; ++t) {
        LmDescDev& r = lrec[(size_t)t];
        TmDescDev& q = trec[(size_t)t];
        r.keys = take((size_t)r.K * 8);
        q.count = take((size_t)r.capacity * 4); q.cursor = take((size_t)r.capacity * 4); q.pairs = take((size_t)q.ocap * 8);
    }
    if (o > (size_t)DSDTM_TRACKMAP_MAX_CALL_BYTES) {
        set_err(ctx, "local: the call's block for %d descs exceeds %lld bytes (8 per keyframe, 45 per point of point_capacity, 48 per observation of obs_capacity)",
                n, (long long)DSDTM_TRACKMAP_MAX_CALL_BYTES);
        return DSDTM_ERR_INVALID;
    }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, o)) return rc;          // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, lrec.data(), N * sizeof(LmDescDev));
    memcpy(h + descs_off, trec.data(), N * sizeof(TmDescDev));
    LmSelectArgs a;
    memset(&a, 0, sizeof a);
    a.block = g; a.n = n; a.max_K = max_K; a.max_P = max_P; a.n_local = prm->n_local; a.boundary = prm->boundary;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.width = cam->width; a.height = cam->height;
    TmLocalArgs f;
    memset(&f, 0, sizeof f);
    f.block = g; f.descs = descs_off; f.n = n; f.max_K = max_K; f.max_cap = max_cap; f.max_ocap = max_ocap;
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(localmap_select_launch(a, ctx->stream));
    API_TRY(trackmap_flatten_launch(f, ctx->stream));
    API_TRY(hipMemcpyAsync(h + out0, g + out0, back - out0, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    for (int t = 0; t < n; ++t) {
        const dsdtm_trackmap_desc& d = descs[t];
        const LmDescDev& r = lrec[(size_t)t];
        const TmDescDev& q = trec[(size_t)t];
        dsdtm_localmap_result sel;
        TmExtResult ext;
        memcpy(&sel, h + r.result, sizeof sel);
        memcpy(&ext, h + q.ext, sizeof ext);
        const size_t n_kf = (size_t)std::min(std::max(sel.n_kf, 0), prm->n_local);
        const size_t m = (size_t)std::min(std::max(sel.n_points, 0), d.point_capacity);
        const size_t n_ob = (size_t)std::min(std::max(ext.n_obs, 0), d.obs_capacity);
        if (n_kf) { memcpy(d.kf, h + r.kf, n_kf * 4); memcpy(d.kf_dist, h + r.kf_dist, n_kf * 8); }
        if (m) {
            memcpy(d.point, h + r.point, m * 4); memcpy(d.point_kf, h + r.point_kf, m * 4);
            memcpy(d.mp_world, h + q.mp_world, m * 24); memcpy(d.mp_found, h + q.mp_found, m * 4); memcpy(d.mp_bad, h + q.mp_bad, m);
        }
        memcpy(d.obs_offset, h + q.obs_offset, (m + 1) * 4);
        if (n_ob) {
            memcpy(d.obs_kf, h + q.obs_kf, n_ob * 4); memcpy(d.obs_px, h + q.obs_px, n_ob * 8);
            memcpy(d.obs_level, h + q.obs_level, n_ob * 4); memcpy(d.obs_bearing, h + q.obs_bearing, n_ob * 24);
        }
        dsdtm_trackmap_result res;
        res.n_close = sel.n_close; res.n_kf = sel.n_kf; res.n_points = sel.n_points; res.n_obs = ext.n_obs;
        res.overflow_points = sel.overflow; res.overflow_obs = ext.overflow_obs;
        results[t] = res;
    }
    return DSDTM_OK;
}
