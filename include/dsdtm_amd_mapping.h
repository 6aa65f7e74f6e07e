/*
 * dsdtm_amd_mapping.h — C ABI of libdsdtm_amd_mapping.so: the MAPPING thread's work on the map that is resident on the MI355X (gfx950):
 * the covisibility list of KeyFrame::UpdateConnection, the window of Optimizer::LocalBundleAdjustment built on the device in the
 * layout dsdtm_local_ba_batch_device takes (include/dsdtm_amd.h), and the commit of the solve with the reference's outlier bookkeeping —
 * window -> solve -> commit, with no column crossing the link. The set construction that include/dsdtm_amd.h leaves with the caller
 * is therefore optional.
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own; the conventions are those of the
 * other add-on headers — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no
 * environment, one context per calling thread, NO CPU fallback. The plain host evaluation of the same rules is update_connection_host,
 * ba_window_host and ba_commit_host (dsdtm_amd/host/dsdtm_mapping_host.hpp), which need no library.
 *
 * THE MAP. This library holds the track map of include/dsdtm_amd_trackmap.h and serves it: the entries dsdtm_mapping_map_create ..
 * dsdtm_mapping_local below have the layouts, the rules and the results of the dsdtm_trackmap_* entries of the same name (ONE
 * implementation, compiled into both libraries), over the same types (dsdtm_trackmap, dsdtm_trackmap_image, dsdtm_trackmap_desc,
 * dsdtm_trackmap_result). A process that runs both threads keeps ONE resident map, this one. A map belongs to the context that made it.
 */
#ifndef DSDTM_AMD_MAPPING_H
#define DSDTM_AMD_MAPPING_H

#include "dsdtm_amd_trackmap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_mapping_ctx dsdtm_mapping_ctx;

int dsdtm_mapping_create(int device, dsdtm_mapping_ctx** out);
void dsdtm_mapping_destroy(dsdtm_mapping_ctx* ctx);
const char* dsdtm_mapping_last_error(const dsdtm_mapping_ctx* ctx);

/* ---- the resident map: see include/dsdtm_amd_trackmap.h, entry for entry ------------------------------------------------------ */
int dsdtm_mapping_map_create(dsdtm_mapping_ctx* ctx, dsdtm_trackmap** out);
void dsdtm_mapping_map_destroy(dsdtm_mapping_ctx* ctx, dsdtm_trackmap* map);
int dsdtm_mapping_points_write(dsdtm_mapping_ctx* ctx, dsdtm_trackmap* map, int first, int n, const double* p_world, const uint8_t* bad,
                               const int32_t* found);
int dsdtm_mapping_found_write(dsdtm_mapping_ctx* ctx, dsdtm_trackmap* map, int n, const int32_t* index, const int32_t* found);
int dsdtm_mapping_keyframe_add(dsdtm_mapping_ctx* ctx, dsdtm_trackmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                               const uint8_t* observes, const float* px_xy, const int32_t* level, const double* bearing, int* out_index);
int dsdtm_mapping_keyframe_write(dsdtm_mapping_ctx* ctx, dsdtm_trackmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                                 const int32_t* point_of_slot, const uint8_t* observes);
int dsdtm_mapping_map_read(dsdtm_mapping_ctx* ctx, const dsdtm_trackmap* map, dsdtm_trackmap_image* out);
int dsdtm_mapping_local(dsdtm_mapping_ctx* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                        const dsdtm_trackmap_desc* descs, dsdtm_trackmap_result* results);

/* ---- KeyFrame::UpdateConnection (src/Keyframe.cpp:71-133) ------------------------------------------------------------------------
 * n (map, keyframe) pairs per call, 0 <= n <= DSDTM_MAPPING_MAX_PAIRS; synchronous.
 * Weights: weight[k] is summed over the slots of `kf` whose point_of_slot is set and whose point is not bad — mvMapPoints is what is
 *   walked (:76-86); the `observes` flag of THAT slot is not consulted, so a slot that lists a point without observing it (the quirk
 *   of include/dsdtm_amd_trackmap.h) still counts. For each such slot every OBSERVING slot of that point in a keyframe k != kf adds 1
 *   (:88-95). A point listed by two slots of kf counts twice.
 * The list: the keyframes with weight > DSDTM_MAPPING_COV_THRESHOLD (:115). If there are none, the single keyframe of largest weight;
 *   among equals the lowest index wins (the `>` of :109 is strict while a map is iterated in order). Sorted ascending by
 *   (weight, keyframe index) (:129): the reference sorts ties by pointer value, index order is this project's definition. No keyframe
 *   with weight > 0: an empty list (:98-99; the caller leaves mOrderedCovGraph as it was).
 * Out: cov_kf / cov_weight (HOST, capacity each; may be NULL when capacity is 0), n_cov = the full count; overflow = n_cov > capacity,
 *   and then the first `capacity` entries of the sorted list are written, whatever the timing. n_connected = the size of mConnectedKFs
 *   (keyframes with weight > 0). Entries behind what a result reports are left untouched.
 * All or nothing: checked on the host before anything is enqueued, DSDTM_ERR_INVALID naming the desc and the field. */
#define DSDTM_MAPPING_COV_THRESHOLD 15
#define DSDTM_MAPPING_MAX_PAIRS 1024
typedef struct dsdtm_mapping_cov_desc {
    const dsdtm_trackmap* map;
    int32_t kf, capacity;
    int32_t* cov_kf; int32_t* cov_weight;
} dsdtm_mapping_cov_desc;
typedef struct dsdtm_mapping_cov_result {
    int32_t n_cov, n_connected, overflow, reserved;
} dsdtm_mapping_cov_result;
int dsdtm_mapping_covisibility(dsdtm_mapping_ctx* ctx, int n, const dsdtm_mapping_cov_desc* descs, dsdtm_mapping_cov_result* results);

/* ---- the window of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:109-159, :166-224) -----------------------------------------
 * n windows per call, 0 <= n <= DSDTM_MAPPING_MAX_WINDOWS; synchronous. No floating-point operation happens anywhere: every value is
 * a copy, bit for bit.
 * Desc: map; kf = tKFrame; cov_kf[n_cov] (HOST) = the caller's stored GetCovKFrames() in ITS order — normally what
 *   dsdtm_mapping_covisibility returned when the keyframe was created; 0 <= n_cov <= DSDTM_MAPPING_MAX_COV; a list that contains kf, a
 *   repeated keyframe or an index outside the map is refused. origin_kf = the map index of the keyframe with mlId == 0, or -1. The
 *   capacities of this window's segments.
 * Arrays: DEVICE pointers, as dsdtm_local_ba_batch_device takes them (T_c2w x12, kf_constant, points x3, obs_kf, obs_point,
 *   obs_bearing x3, obs_level), plus kf_index (window keyframe -> map keyframe), point_index (window point -> map point) and obs_slot
 *   (observation -> (map keyframe << 32 | slot)). Window w's segment of each array starts at the SUM of the earlier windows'
 *   capacities (keyframe_capacity, point_capacity, observation_capacity), so the offsets are known before anything runs; they are
 *   what problems[w] holds. h_kf_index, h_point_index, h_obs_slot: HOST arrays of the same layout and the same total size, each may
 *   be NULL; the three device index arrays are copied there WHOLE (the host needs them to mirror the bookkeeping on its objects; what
 *   lies behind a window's counts, and the segment of a window that is not usable, is as unspecified there as on the device).
 * W1 local keyframes: kf, then cov_kf in the given order (:110-121). kf_constant = 1 only for a local keyframe that is origin_kf (:182-183).
 * W2 local points: for the local keyframes in W1 order, slots in slot order, each listed (point_of_slot set; `observes` not consulted),
 *   non-bad point at its first occurrence (:123-141). QUIRK, kept: a window with kf == origin_kf collects NO points — mlLocalBAKFId
 *   starts at 0 (src/MapPoint.cpp:20), so the test of :135 fails for every point. The marks the reference leaves on its objects
 *   (mlLocalBAKFId, mlLocalBAKfId, mlFixedLocalBAKfId) are otherwise not state here: the window is what the reference builds THE FIRST
 *   TIME it is asked for that keyframe.
 * W3 fixed keyframes: for the local points in W2 order, their observing slots over ALL keyframes of the map in ascending (keyframe,
 *   slot) order; each keyframe that is not local is taken at its first occurrence (:143-159). Fixed keyframes are constant and follow
 *   the local ones.
 * W4 observations: points in W2 order, each with all its observing slots in ascending (keyframe, slot) order (this project's order: the
 *   reference iterates by pointer value). By W3 every observer is in the window. obs_kf / obs_point are window-local, obs_point does
 *   not decrease; bearing and level are the slot's feature columns, T_c2w and points the map's.
 * Result: the full counts n_local, n_fixed, n_points, n_obs; one flag per limit or capacity that was exceeded —
 *   over_free_kf (free keyframes > DSDTM_LBA_MAX_FREE_KF), over_const_kf (constant ones > DSDTM_LBA_MAX_CONST_KF), over_points
 *   (> DSDTM_LBA_MAX_POINTS), over_obs (> DSDTM_LBA_MAX_OBSERVATIONS), over_keyframe_capacity, over_point_capacity,
 *   over_observation_capacity —; usable = 1 only when no flag is set and there is at least one free keyframe.
 *   A window that is not usable MUST NOT be handed to the solver (the caller takes its host path for it): its
 *   problems[w] has all counts 0 and the contents of its segments are unspecified. HAND ON THE USABLE WINDOWS ONLY:
 *   dsdtm_local_ba_batch_device refuses a problem without a free keyframe.
 * All or nothing: everything is checked on the host before anything is enqueued; DSDTM_ERR_INVALID names the desc and the field,
 *   outputs untouched. A HIP call that fails BEHIND the first enqueue (DSDTM_ERR_HIP) leaves problems and results untouched, but the
 *   device arrays, and the host index arrays, may already be written in part: their contents are then unspecified. A call whose device block would exceed DSDTM_TRACKMAP_MAX_CALL_BYTES is refused (24 bytes per slot of the local
 *   keyframes, 8 per keyframe of the map, 8 per observation of observation_capacity). */
#define DSDTM_MAPPING_MAX_WINDOWS 256
#define DSDTM_MAPPING_MAX_COV 255
typedef struct dsdtm_mapping_window_desc {
    const dsdtm_trackmap* map;
    int32_t kf, n_cov;
    const int32_t* cov_kf;
    int32_t origin_kf;
    int32_t keyframe_capacity, point_capacity, observation_capacity;
} dsdtm_mapping_window_desc;
typedef struct dsdtm_mapping_window_arrays {
    double* T_c2w; uint8_t* kf_constant; double* points;                               /* device */
    int32_t* obs_kf; int32_t* obs_point; double* obs_bearing; int32_t* obs_level;      /* device */
    int32_t* kf_index; int32_t* point_index; int64_t* obs_slot;                        /* device */
    int32_t* h_kf_index; int32_t* h_point_index; int64_t* h_obs_slot;                  /* host, each may be NULL */
} dsdtm_mapping_window_arrays;
typedef struct dsdtm_mapping_window_result {
    int32_t n_local, n_fixed, n_points, n_obs;
    int32_t over_free_kf, over_const_kf, over_points, over_obs;
    int32_t over_keyframe_capacity, over_point_capacity, over_observation_capacity;
    int32_t usable;
} dsdtm_mapping_window_result;
int dsdtm_mapping_ba_window(dsdtm_mapping_ctx* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_mapping_window_arrays* arrays,
                            dsdtm_local_ba_problem* problems, dsdtm_mapping_window_result* results);

/* ---- the commit of a solved window (src/Optimizer.cpp:236-271, src/MapPoint.cpp:57-109) --------------------------------------------
 * Takes the windows of ONE dsdtm_mapping_ba_window call — the same descs, problems, results and arrays, T_c2w and points now holding
 * the solver's output — with the solver's DEVICE outlier array (problem w's flags at observation_offset) and the hip_stream the solve
 * was enqueued on: the commit is ordered behind that stream's work on the device and in front of every later call on this context.
 * Synchronous. Windows with usable == 0 are skipped (their result is all 0).
 * C1 every window keyframe's pose, constant ones included, and every window point's position are written into the map (:236-248).
 * C2 the outlier pass, replayed exactly. Per point, n0 = its observation count (mObsNum: under THE CALLER'S DUTY of
 *   include/dsdtm_amd_trackmap.h, the number of its observing slots); its outliers are taken in observation order. The j-th outlier
 *   (j = 1, 2, ...) has its `observes` cleared and its point_of_slot KEPT (Erase_Observation, then Erase_MapPointMatch(MapPoint*)
 *   finds no index, :266-267). As soon as n0 - j <= 1 the point goes bad (Erase_Observation -> SetBadFlag, src/MapPoint.cpp:74-80):
 *   every observing slot that is still left — later outliers and non-outliers alike — gets observes = 0 AND point_of_slot = -1
 *   (src/MapPoint.cpp:98-105), and bad = 1. Later outliers of that point change nothing, but still count in n_outliers (:269).
 *   The work is per point and independent; no result depends on arrival order.
 * Out per window: n_outliers; n_bad and bad_points (HOST, n x bad_capacity; window w's at w * bad_capacity; may be NULL when
 *   bad_capacity is 0): the MAP indices of the points that went bad, in window point order; overflow_bad = n_bad > bad_capacity (the
 *   first bad_capacity are written). The caller reads the outlier array itself if it wants the flags.
 * OVERLAP: the usable windows of one call must not share a keyframe (local or fixed) or a point of one map: solved independently they
 *   would overwrite each other. Found on the device before anything is written; DSDTM_ERR_INVALID naming both windows, the map unchanged. */
typedef struct dsdtm_mapping_commit_result {
    int32_t n_outliers, n_bad, overflow_bad, reserved;
} dsdtm_mapping_commit_result;
int dsdtm_mapping_ba_commit(dsdtm_mapping_ctx* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_local_ba_problem* problems,
                            const dsdtm_mapping_window_result* results, const dsdtm_mapping_window_arrays* arrays, const uint8_t* outlier,
                            void* hip_stream, int bad_capacity, int32_t* bad_points, dsdtm_mapping_commit_result* out);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_MAPPING_H */
