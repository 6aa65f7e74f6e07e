// mapping_api_body.h — the three entries of the mapping thread (include/dsdtm_amd_mapping.h): the checks and the packing of a
// covisibility, a window and a commit call. ONE implementation, compiled once per library that serves them: the including translation
// unit names the entries (MP_API(ba_window) -> dsdtm_mapping_ba_window in mapping_api.cpp, dsdtm_slam_ba_window in slam_api.cpp) and
// includes trackmap_api_body.h (the map, the context TM_CTX and its staging) in front of this file. Each entry is one upload (the descs
// as the device sees them, with the offsets of outputs and temporaries in the call's device block), the launches of mapping.hip, one
// read-back, one wait (the commit waits twice: for the overlap verdict, then for the results). There is no CPU compute path here (the
// host evaluation is host/dsdtm_mapping_host.hpp, which needs no library).
#if !defined(MP_API) || !defined(DSDTM_TRACKMAP_API_BODY_H)
#error "mapping_api_body.h: define MP_API(name) and include trackmap_api_body.h before including it (see mapping_api.cpp)"
#endif
#ifdef DSDTM_MAPPING_API_BODY_H
#error "mapping_api_body.h defines the entries of ONE library: include it once per translation unit"
#endif
#define DSDTM_MAPPING_API_BODY_H
#include "mapping.h"

// what one call's block is laid out with: the next 8-aligned offset
struct Taker {
    size_t o;
    uint64_t operator()(size_t bytes) { const size_t at = o; o = align_up(o + bytes, 8); return (uint64_t)at; }
};

extern "C" int MP_API(covisibility)(TM_CTX* ctx,int n, const dsdtm_mapping_cov_desc* descs, dsdtm_mapping_cov_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MAPPING_MAX_PAIRS) { set_err(ctx, "covisibility: n = %d outside 0..%d", n, DSDTM_MAPPING_MAX_PAIRS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs || !results) { set_err(ctx, "covisibility: %s is NULL", !descs ? "descs" : "results"); return DSDTM_ERR_INVALID; }
    const size_t N = (size_t)n;
    std::vector<MpCovDev> rec(N);
    Taker take{align_up(N * sizeof(MpCovDev), 16)};
    const size_t up = take.o;
    int max_K = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_mapping_cov_desc& d = descs[t];
        const char* bad = nullptr;
        if (!d.map) bad = "map is NULL";
        else if (!owns(ctx, d.map)) bad = "map is not a map of this context";
        else if (d.kf < 0 || (int64_t)d.kf >= d.map->used[1]) bad = "kf is not a keyframe of the map";
        else if (d.capacity < 0 || d.capacity > DSDTM_LOCALMAP_MAX_KEYFRAMES) bad = "capacity out of range";
        else if (d.capacity > 0 && !d.cov_kf) bad = "cov_kf is NULL";
        else if (d.capacity > 0 && !d.cov_weight) bad = "cov_weight is NULL";
        if (bad) { set_err(ctx, "covisibility: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        MpCovDev& r = rec[(size_t)t];
        memset(&r, 0, sizeof r);
        r.points = d.map->d_points; r.kfs = d.map->d_kfs; r.slots = d.map->d_slots; r.obs = d.map->d_obs;
        r.K = (int32_t)d.map->used[1]; r.kf = d.kf; r.capacity = d.capacity;
        max_K = std::max(max_K, r.K);
        r.result = take(sizeof(dsdtm_mapping_cov_result)); r.cov_kf = take((size_t)d.capacity * 4); r.cov_weight = take((size_t)d.capacity * 4);
    }
    const size_t back = align_up(take.o, 256);
    take.o = back;
    for (MpCovDev& r : rec) r.weight = take((size_t)r.K * 4);
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, take.o)) return rc;
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, rec.data(), N * sizeof(MpCovDev));
    MpCovArgs a;
    memset(&a, 0, sizeof a);
    a.block = g; a.n = n; a.max_K = max_K;
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, N * sizeof(MpCovDev), hipMemcpyHostToDevice, ctx->stream));
    API_TRY(mapping_covisibility_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + up, g + up, back - up, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    stream_idle(ctx);
    for (int t = 0; t < n; ++t) {
        const MpCovDev& r = rec[(size_t)t];
        dsdtm_mapping_cov_result res;
        memcpy(&res, h + r.result, sizeof res);
        const size_t m = (size_t)std::min(std::max(res.n_cov, 0), descs[t].capacity);
        if (m) { memcpy(descs[t].cov_kf, h + r.cov_kf, m * 4); memcpy(descs[t].cov_weight, h + r.cov_weight, m * 4); }
        results[t] = res;
    }
    return DSDTM_OK;
}

// the capacities of window t summed over the windows in front of it
struct Offsets { int64_t kf, point, obs; };

static const char* bad_window_desc(const TM_CTX* ctx, const dsdtm_mapping_window_desc& d, std::vector<uint8_t>& seen) {
    if (!d.map) return "map is NULL";
    if (!owns(ctx, d.map)) return "map is not a map of this context";
    const int64_t K = d.map->used[1];
    if (d.kf < 0 || (int64_t)d.kf >= K) return "kf is not a keyframe of the map";
    if (d.n_cov < 0 || d.n_cov > DSDTM_MAPPING_MAX_COV) return "n_cov out of range";
    if (d.n_cov > 0 && !d.cov_kf) return "cov_kf is NULL";
    if (d.origin_kf < -1 || (int64_t)d.origin_kf >= K) return "origin_kf is neither -1 nor a keyframe of the map";
    if (d.keyframe_capacity < 0 || d.point_capacity < 0 || d.observation_capacity < 0) return "a capacity is negative";
    if (d.keyframe_capacity > DSDTM_LBA_MAX_FREE_KF + DSDTM_LBA_MAX_CONST_KF) return "keyframe_capacity exceeds what a problem takes";
    if (d.point_capacity > DSDTM_LBA_MAX_POINTS) return "point_capacity exceeds DSDTM_LBA_MAX_POINTS";
    if (d.observation_capacity > DSDTM_LBA_MAX_OBSERVATIONS) return "observation_capacity exceeds DSDTM_LBA_MAX_OBSERVATIONS";
    seen.assign((size_t)K, 0);
    seen[(size_t)d.kf] = 1;
    for (int i = 0; i < d.n_cov; ++i) {
        const int k = d.cov_kf[i];
        if (k < 0 || (int64_t)k >= K) return "cov_kf holds an index outside the map";
        if (k == d.kf) return "cov_kf contains kf";
        if (seen[(size_t)k]) return "cov_kf repeats a keyframe";
        seen[(size_t)k] = 1;
    }
    return nullptr;
}

static const char* missing_array(const dsdtm_mapping_window_arrays& a, int64_t kfs, int64_t points, int64_t obs) {
    return kfs && !a.T_c2w ? "T_c2w" : kfs && !a.kf_constant ? "kf_constant" : kfs && !a.kf_index ? "kf_index" : points && !a.points ? "points"
         : points && !a.point_index ? "point_index" : obs && !a.obs_kf ? "obs_kf" : obs && !a.obs_point ? "obs_point" : obs && !a.obs_bearing ? "obs_bearing"
         : obs && !a.obs_level ? "obs_level" : obs && !a.obs_slot ? "obs_slot" : nullptr;
}

extern "C" int MP_API(ba_window)(TM_CTX* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_mapping_window_arrays* arrays,
                                 dsdtm_local_ba_problem* problems, dsdtm_mapping_window_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MAPPING_MAX_WINDOWS) { set_err(ctx, "ba_window: n = %d outside 0..%d", n, DSDTM_MAPPING_MAX_WINDOWS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    const char* null_arg = !descs ? "descs" : !arrays ? "arrays" : !problems ? "problems" : !results ? "results" : nullptr;
    if (null_arg) { set_err(ctx, "ba_window: %s is NULL", null_arg); return DSDTM_ERR_INVALID; }
    const size_t N = (size_t)n;
    std::vector<MpWinDev> rec(N);
    std::vector<Offsets> offs(N);
    std::vector<uint8_t> seen;
    std::vector<int32_t> lists;                 // per window: its local keyframes, then its n_local + 1 entry offsets
    Offsets sum{0, 0, 0};
    for (int t = 0; t < n; ++t) {
        const dsdtm_mapping_window_desc& d = descs[t];
        if (const char* bad = bad_window_desc(ctx, d, seen)) { set_err(ctx, "ba_window: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        offs[(size_t)t] = sum;
        sum.kf += d.keyframe_capacity; sum.point += d.point_capacity; sum.obs += d.observation_capacity;
    }
    if (const char* missing = missing_array(*arrays, sum.kf, sum.point, sum.obs)) { set_err(ctx, "ba_window: arrays: %s is NULL", missing); return DSDTM_ERR_INVALID; }
    Taker take{align_up(N * sizeof(MpWinDev), 16)};
    int max_K = 0, max_E = 0, max_T = 0, max_ocap = 0;
    for (int t = 0; t < n; ++t) {
        const dsdtm_mapping_window_desc& d = descs[t];
        const Offsets& at = offs[(size_t)t];
        MpWinDev& r = rec[(size_t)t];
        memset(&r, 0, sizeof r);
        r.points = d.map->d_points; r.kfs = d.map->d_kfs; r.slots = d.map->d_slots; r.obs = d.map->d_obs; r.feat = d.map->d_feat;
        r.K = (int32_t)d.map->used[1]; r.P = (int32_t)d.map->used[0]; r.kf = d.kf; r.origin = d.origin_kf; r.n_local = 1 + d.n_cov;
        r.kcap = d.keyframe_capacity; r.pcap = d.point_capacity; r.ocap = d.observation_capacity;
        const size_t first = lists.size();
        lists.push_back(d.kf);
        lists.insert(lists.end(), d.cov_kf, d.cov_kf + d.n_cov);
        int64_t E = 0;
        for (int i = 0; i <= d.n_cov; ++i) {
            lists.push_back((int32_t)E);
            E += d.map->kf_n_slots[(size_t)lists[first + (size_t)i]];
        }
        lists.push_back((int32_t)E);    // (n_local + 1 offsets: the last one is E; at most 256 x 4096 entries)
        r.E = (int32_t)E;
        r.T_bits = 4;
        while ((1ll << r.T_bits) < 2 * E) ++r.T_bits;
        r.T_c2w = arrays->T_c2w + 12 * at.kf; r.kf_constant = arrays->kf_constant + at.kf; r.kf_index = arrays->kf_index + at.kf;
        r.pts = arrays->points + 3 * at.point; r.point_index = arrays->point_index + at.point;
        r.obs_kf = arrays->obs_kf + at.obs; r.obs_point = arrays->obs_point + at.obs; r.obs_bearing = arrays->obs_bearing + 3 * at.obs;
        r.obs_level = arrays->obs_level + at.obs; r.obs_slot = arrays->obs_slot + at.obs;
        r.local = take((size_t)r.n_local * 4); r.ent_off = take(((size_t)r.n_local + 1) * 4);
        max_K = std::max(max_K, r.K); max_E = std::max(max_E, r.E); max_T = std::max(max_T, 1 << r.T_bits); max_ocap = std::max(max_ocap, r.ocap);
    }
    const size_t up = align_up(take.o, 16);
    take.o = up;
    for (MpWinDev& r : rec) r.result = take(sizeof(dsdtm_mapping_window_result));
    const size_t back = align_up(take.o, 256);
    take.o = back;
    for (MpWinDev& r : rec) {
        const size_t T = (size_t)1 << r.T_bits, E = (size_t)r.E;
        r.table = take(T * 8); r.cell_lp = take(T * 4); r.count = take(E * 4); r.cursor = take(E * 4); r.off = take((E + 1) * 4);
        r.kfkey = take((size_t)r.K * 4); r.kfwin = take((size_t)r.K * 4); r.pairs = take((size_t)r.ocap * 8);
        if (take.o > (size_t)DSDTM_TRACKMAP_MAX_CALL_BYTES) {
            set_err(ctx, "ba_window: the call's block for %d windows exceeds %lld bytes (24 per slot of the local keyframes, 8 per keyframe, 8 per observation of observation_capacity)",
                    n, (long long)DSDTM_TRACKMAP_MAX_CALL_BYTES);
            return DSDTM_ERR_INVALID;
        }
    }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, take.o)) return rc;      // (first: it may wait for the stream and hand the pinned block back)
    if (int rc = pinned_reserve(ctx, back, &h)) return rc;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, rec.data(), N * sizeof(MpWinDev));
    {
        size_t at = 0;
        for (const MpWinDev& r : rec) {
            memcpy(h + r.local, lists.data() + at, (size_t)r.n_local * 4);
            memcpy(h + r.ent_off, lists.data() + at + (size_t)r.n_local, ((size_t)r.n_local + 1) * 4);
            at += 2 * (size_t)r.n_local + 1;
        }
    }
    MpWinArgs a;
    memset(&a, 0, sizeof a);
    a.block = g; a.n = n; a.max_K = max_K; a.max_E = max_E; a.max_T = max_T; a.max_ocap = max_ocap;
    auto fail = [&](int rc) { if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(mapping_window_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + up, g + up, back - up, hipMemcpyDeviceToHost, ctx->stream));
    // the index arrays for the host, where it asked for them: each device array whole, behind the launches on the same stream (at most
    // three copies per call; pageable destinations: the call is synchronous). A copy that fails leaves problems and results untouched.
    if (arrays->h_kf_index && sum.kf) API_TRY(hipMemcpyAsync(arrays->h_kf_index, arrays->kf_index, (size_t)sum.kf * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (arrays->h_point_index && sum.point) API_TRY(hipMemcpyAsync(arrays->h_point_index, arrays->point_index, (size_t)sum.point * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (arrays->h_obs_slot && sum.obs) API_TRY(hipMemcpyAsync(arrays->h_obs_slot, arrays->obs_slot, (size_t)sum.obs * 8, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<dsdtm_mapping_window_result> res(N);
    for (int t = 0; t < n; ++t) memcpy(&res[(size_t)t], h + rec[(size_t)t].result, sizeof res[0]);
    stream_idle(ctx);
    for (int t = 0; t < n; ++t) {
        const dsdtm_mapping_window_result& r = res[(size_t)t];
        const Offsets& at = offs[(size_t)t];
        dsdtm_local_ba_problem p;
        memset(&p, 0, sizeof p);
        if (r.usable) { p.n_keyframes = r.n_local + r.n_fixed; p.n_points = r.n_points; p.n_observations = r.n_obs; }
        p.keyframe_offset = at.kf; p.point_offset = at.point; p.observation_offset = at.obs;
        problems[t] = p;
        results[t] = r;
    }
    return DSDTM_OK;
}

extern "C" int MP_API(ba_commit)(TM_CTX* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_local_ba_problem* problems,
                                 const dsdtm_mapping_window_result* results, const dsdtm_mapping_window_arrays* arrays, const uint8_t* outlier,
                                 void* hip_stream, int bad_capacity, int32_t* bad_points, dsdtm_mapping_commit_result* out) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_MAPPING_MAX_WINDOWS) { set_err(ctx, "ba_commit: n = %d outside 0..%d", n, DSDTM_MAPPING_MAX_WINDOWS); return DSDTM_ERR_INVALID; }
    if (bad_capacity < 0 || bad_capacity > DSDTM_LBA_MAX_POINTS) { set_err(ctx, "ba_commit: bad_capacity = %d outside 0..%d", bad_capacity, DSDTM_LBA_MAX_POINTS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    const char* null_arg = !descs ? "descs" : !problems ? "problems" : !results ? "results" : !arrays ? "arrays" : !out ? "out"
                         : bad_capacity > 0 && !bad_points ? "bad_points" : nullptr;
    if (null_arg) { set_err(ctx, "ba_commit: %s is NULL", null_arg); return DSDTM_ERR_INVALID; }
    std::vector<MpCommitDev> rec;
    std::vector<const dsdtm_trackmap*> maps;    // the distinct maps of the usable windows
    std::vector<size_t> map_of;
    std::vector<uint8_t> seen;
    Offsets sum{0, 0, 0};
    for (int t = 0; t < n; ++t) {
        const dsdtm_mapping_window_desc& d = descs[t];
        const dsdtm_local_ba_problem& p = problems[t];
        const char* bad = bad_window_desc(ctx, d, seen);
        if (!bad && (p.keyframe_offset != sum.kf || p.point_offset != sum.point || p.observation_offset != sum.obs)) bad = "problems: the offsets are not the sums of the earlier capacities";
        if (!bad && results[t].usable && (p.n_keyframes < 1 || p.n_keyframes > d.keyframe_capacity || p.n_points < 0 || p.n_points > d.point_capacity ||
                                          p.n_observations < 0 || p.n_observations > d.observation_capacity)) bad = "problems: a count exceeds its capacity";
        if (bad) { set_err(ctx, "ba_commit: desc %d: %s", t, bad); return DSDTM_ERR_INVALID; }
        const Offsets at = sum;
        sum.kf += d.keyframe_capacity; sum.point += d.point_capacity; sum.obs += d.observation_capacity;
        if (!results[t].usable) continue;
        MpCommitDev r;
        memset(&r, 0, sizeof r);
        r.points = d.map->d_points; r.kfs = d.map->d_kfs; r.slots = d.map->d_slots; r.obs = d.map->d_obs;
        r.K = (int32_t)d.map->used[1]; r.P = (int32_t)d.map->used[0];
        r.n_kf = p.n_keyframes; r.n_points = p.n_points; r.n_obs = p.n_observations; r.window = t; r.bad_cap = bad_capacity;
        r.T_c2w = arrays->T_c2w + 12 * at.kf; r.kf_index = arrays->kf_index + at.kf;
        r.pts = arrays->points + 3 * at.point; r.point_index = arrays->point_index + at.point;
        r.obs_point = arrays->obs_point + at.obs; r.obs_slot = arrays->obs_slot + at.obs; r.outlier = outlier + at.obs;
        size_t m = std::find(maps.begin(), maps.end(), d.map) - maps.begin();
        if (m == maps.size()) maps.push_back(d.map);
        map_of.push_back(m);
        rec.push_back(r);
    }
    if (const char* missing = missing_array(*arrays, sum.kf, sum.point, sum.obs)) { set_err(ctx, "ba_commit: arrays: %s is NULL", missing); return DSDTM_ERR_INVALID; }
    if (sum.obs && !outlier) { set_err(ctx, "ba_commit: outlier is NULL"); return DSDTM_ERR_INVALID; }
    for (int t = 0; t < n; ++t) memset(&out[t], 0, sizeof out[t]);
    if (rec.empty()) return DSDTM_OK;
    const size_t M = rec.size();
    Taker take{align_up(M * sizeof(MpCommitDev), 16)};
    const size_t up = take.o;
    int max_items = 1;
    for (MpCommitDev& r : rec) {
        r.result = take(sizeof(dsdtm_mapping_commit_result)); r.bad_list = take((size_t)bad_capacity * 4);
        max_items = std::max({max_items, r.n_kf, r.n_points});
    }
    const size_t back = align_up(take.o, 256);
    take.o = back;
    MpCommitArgs a;
    memset(&a, 0, sizeof a);
    a.verdict = take(8);
    a.claims = take.o;
    std::vector<uint64_t> claim_k(maps.size()), claim_p(maps.size());
    for (size_t m = 0; m < maps.size(); ++m) {      // (4-byte steps: the fill runs over the verdict and every claim array as one run of words)
        claim_k[m] = take.o; take.o += (size_t)maps[m]->used[1] * 4;
        claim_p[m] = take.o; take.o += (size_t)maps[m]->used[0] * 4;
    }
    a.claim_words = (take.o - a.verdict) / 4;
    take.o = align_up(take.o, 8);
    for (size_t i = 0; i < M; ++i) {
        MpCommitDev& r = rec[i];
        r.claim_k = claim_k[map_of[i]]; r.claim_p = claim_p[map_of[i]];
        r.went_bad = take((size_t)r.n_points * 4); r.n_out = take((size_t)r.n_points * 4);
    }
    uint8_t* h = nullptr;
    if (int rc = device_stage_reserve(ctx, take.o)) return rc;
    if (int rc = pinned_reserve(ctx, back + 256, &h)) return rc;      // (+ the verdict's landing place)
    uint8_t* g = (uint8_t*)ctx->d_stage;
    memcpy(h, rec.data(), M * sizeof(MpCommitDev));
    a.block = g; a.n = (int)M; a.max_items = max_items;
    // behind the solve: this context's stream waits for what the solver's stream holds now
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t solved = nullptr;
    HIP_TRY(ctx, hipEventCreateWithFlags(&solved, hipEventDisableTiming));
    auto fail = [&](int rc) { if (solved) { (void)hipEventDestroy(solved); solved = nullptr; } if (hipStreamSynchronize(ctx->stream) == hipSuccess) stream_idle(ctx); return rc; };
    API_TRY(hipEventRecord(solved, (hipStream_t)hip_stream));
    API_TRY(hipStreamWaitEvent(ctx->stream, solved, 0));
    API_TRY(hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(mapping_commit_check_launch(a, ctx->stream));
    unsigned long long* verdict = (unsigned long long*)(h + back);
    API_TRY(hipMemcpyAsync(verdict, g + a.verdict, 8, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    (void)hipEventDestroy(solved);
    solved = nullptr;
    if (*verdict != MP_NO_OVERLAP) {
        set_err(ctx, "ba_commit: windows %d and %d share a keyframe or a point of their map; nothing was written", (int)(*verdict >> 32), (int)(*verdict & 0xffffffffull));
        stream_idle(ctx);
        return DSDTM_ERR_INVALID;
    }
    API_TRY(mapping_commit_apply_launch(a, ctx->stream));
    API_TRY(hipMemcpyAsync(h + up, g + up, back - up, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (const MpCommitDev& r : rec) {
        dsdtm_mapping_commit_result res;
        memcpy(&res, h + r.result, sizeof res);
        const size_t m = (size_t)std::min(std::max(res.n_bad, 0), bad_capacity);
        if (m) memcpy(bad_points + (size_t)r.window * (size_t)bad_capacity, h + r.bad_list, m * 4);
        out[r.window] = res;
    }
    stream_idle(ctx);
    return DSDTM_OK;
}
