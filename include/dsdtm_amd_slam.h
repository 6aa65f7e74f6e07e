/*
 * dsdtm_amd_slam.h — C ABI of libdsdtm_amd_slam.so: ONE resident map on the MI355X (gfx950) for the whole per-frame loop — the local
 * map of a tracked frame, the mapping thread's covisibility list, local-BA window and commit, and what closes the loop: the side
 * effects of a TRACKED FRAME on the map (MapPoint::IncreaseFound, the EraseFound walk of Optimizer::PoseOptimization and the
 * SetBadFlag cascade), applied on the device by dsdtm_slam_track_commit. Without it the found counts, which order the candidates of
 * the next frame's cell walk, and the bad flags of the resident map are true for one frame only.
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own; the conventions are those of the
 * other add-on headers — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no
 * environment, one context per calling thread, NO CPU fallback. The plain host evaluation of the rules below is track_commit_host
 * (dsdtm_amd/host/dsdtm_slam_host.hpp), which needs no library.
 *
 * THE MAP. A map belongs to the context that made it and a process keeps ONE resident map, so this library is a SUPERSET of
 * libdsdtm_amd_mapping.so the way that library is a superset of libdsdtm_amd_trackmap.so: the entries dsdtm_slam_map_create ..
 * dsdtm_slam_local have the layouts, the rules and the results of the dsdtm_trackmap_* entries of the same name, and
 * dsdtm_slam_covisibility, _ba_window and _ba_commit those of the dsdtm_mapping_* entries of the same name (ONE implementation each,
 * compiled into every library that serves it), over the same types. The older libraries (libdsdtm_amd_localmap.so,
 * libdsdtm_amd_trackmap.so, libdsdtm_amd_mapping.so) remain for callers who want one stage alone.
 */
#ifndef DSDTM_AMD_SLAM_H
#define DSDTM_AMD_SLAM_H

#include "dsdtm_amd_keyframe.h"
#include "dsdtm_amd_mapping.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_slam_ctx dsdtm_slam_ctx;

int dsdtm_slam_create(int device, dsdtm_slam_ctx** out);
void dsdtm_slam_destroy(dsdtm_slam_ctx* ctx);
const char* dsdtm_slam_last_error(const dsdtm_slam_ctx* ctx);

/* ---- the resident map: see include/dsdtm_amd_trackmap.h, entry for entry ------------------------------------------------------ */
int dsdtm_slam_map_create(dsdtm_slam_ctx* ctx, dsdtm_trackmap** out);
void dsdtm_slam_map_destroy(dsdtm_slam_ctx* ctx, dsdtm_trackmap* map);
int dsdtm_slam_points_write(dsdtm_slam_ctx* ctx, dsdtm_trackmap* map, int first, int n, const double* p_world, const uint8_t* bad,
                            const int32_t* found);
int dsdtm_slam_found_write(dsdtm_slam_ctx* ctx, dsdtm_trackmap* map, int n, const int32_t* index, const int32_t* found);
int dsdtm_slam_keyframe_add(dsdtm_slam_ctx* ctx, dsdtm_trackmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                            const uint8_t* observes, const float* px_xy, const int32_t* level, const double* bearing, int* out_index);
int dsdtm_slam_keyframe_write(dsdtm_slam_ctx* ctx, dsdtm_trackmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                              const int32_t* point_of_slot, const uint8_t* observes);
int dsdtm_slam_map_read(dsdtm_slam_ctx* ctx, const dsdtm_trackmap* map, dsdtm_trackmap_image* out);
int dsdtm_slam_local(dsdtm_slam_ctx* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                     const dsdtm_trackmap_desc* descs, dsdtm_trackmap_result* results);

/* ---- the mapping thread: see include/dsdtm_amd_mapping.h, entry for entry ------------------------------------------------------ */
int dsdtm_slam_covisibility(dsdtm_slam_ctx* ctx, int n, const dsdtm_mapping_cov_desc* descs, dsdtm_mapping_cov_result* results);
int dsdtm_slam_ba_window(dsdtm_slam_ctx* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_mapping_window_arrays* arrays,
                         dsdtm_local_ba_problem* problems, dsdtm_mapping_window_result* results);
int dsdtm_slam_ba_commit(dsdtm_slam_ctx* ctx, int n, const dsdtm_mapping_window_desc* descs, const dsdtm_local_ba_problem* problems,
                         const dsdtm_mapping_window_result* results, const dsdtm_mapping_window_arrays* arrays, const uint8_t* outlier,
                         void* hip_stream, int bad_capacity, int32_t* bad_points, dsdtm_mapping_commit_result* out);

/* ---- a tracked frame's effects on the map (src/Feature_alignment.cpp:106, src/Optimizer.cpp:81-94, src/MapPoint.cpp:91-109, :183-198)
 * n tracked frames per call, 0 <= n <= DSDTM_LOCALMAP_MAX_DESCS; n == 0: DSDTM_OK, nothing done. Synchronous: one upload, the
 * launches, one read-back, one wait. The commit is ordered in front of every later call on the context: a dsdtm_slam_local issued
 * next sees the new counts and flags.
 * Desc: map; n_matches in 0..DSDTM_SLAM_MAX_MATCHES (0: a lost frame); point[n_matches] (HOST): the MAP index of each match of
 *   SearchLocalPoints — point_list[ms[k].point] of the list dsdtm_slam_local returned; residual_norm[n_matches] (HOST): the doubles
 *   dsdtm_track_frame(s) returns; found_after[n_matches] (HOST, may be NULL): the found count of point[i] after this desc was applied.
 *   outlier_threshold is the caller's tOutlineThres (src/Optimizer.cpp:22-24), shared by the call.
 * T1 every match does found[p] += 1 (MapPoint::IncreaseFound, src/Feature_alignment.cpp:106), whether p is bad or not.
 * T2 behind ALL of the desc's T1, in match order: a match with residual_norm[i] > outlier_threshold (strictly; a NaN norm erases
 *   nothing) whose point is not bad does found[p] -= 1 (MapPoint::EraseFound, src/Optimizer.cpp:84-92; counted in n_erased), and when
 *   the count is now <= 0 the point goes bad (src/MapPoint.cpp:191-197).
 * T3 a point that goes bad IN THIS CALL: bad = 1, and every OBSERVING slot of it, in every keyframe of the map, gets observes = 0 and
 *   point_of_slot = -1 (MapPoint::SetBadFlag -> KeyFrame::Erase_MapPointMatch, src/MapPoint.cpp:98-105). A slot that lists the point
 *   without observing it keeps it (the local-BA quirk of include/dsdtm_amd_trackmap.h: it is not in mObservations, so SetBadFlag does
 *   not reach it). A point that was bad before the call, however its slots were written, is not touched by the cascade.
 * T4 descs on the same map are applied in desc order, each wholly before the next (the lockstep loop of INTEGRATION §5c): a point that
 *   desc 0 turned bad is still incremented by desc 1 but no longer erased. Descs on different maps are independent. No result depends
 *   on arrival order or timing.
 * Out per desc: n_erased; n_bad and bad_points (HOST, n x bad_capacity; desc t's at t * bad_capacity; may be NULL when bad_capacity
 *   is 0): the MAP indices of the points that went bad through desc t, in match order; overflow_bad = n_bad > bad_capacity (the first
 *   bad_capacity are written). Entries behind what a result reports are left untouched.
 * All or nothing: checked on the host before anything is enqueued, DSDTM_ERR_INVALID naming the desc and the field, the map and the
 *   outputs untouched — a NULL argument, a map of another context, n_matches outside its range, a point index outside the map, THE SAME
 *   POINT TWICE IN ONE DESC (a frame projects each map point once, src/Tracking.cpp:294-297), a threshold that is not finite, a
 *   negative bad_capacity. The same map may appear in several descs. A HIP call that fails BEHIND the first enqueue (DSDTM_ERR_HIP)
 *   leaves results, bad_points and found_after untouched, but the map may already be written: the caller reads it back
 *   (dsdtm_slam_map_read) or rebuilds it. */
#define DSDTM_SLAM_MAX_MATCHES 256
typedef struct dsdtm_slam_commit_desc {
    dsdtm_trackmap* map;
    int32_t n_matches, reserved;
    const int32_t* point;
    const double* residual_norm;
    int32_t* found_after;
} dsdtm_slam_commit_desc;
typedef struct dsdtm_slam_commit_result {
    int32_t n_erased, n_bad, overflow_bad, reserved;
} dsdtm_slam_commit_result;
int dsdtm_slam_track_commit(dsdtm_slam_ctx* ctx, double outlier_threshold, int n, const dsdtm_slam_commit_desc* descs, int bad_capacity,
                            int32_t* bad_points, dsdtm_slam_commit_result* results);

/* ---- Tracking::NeedKeyframe on the resident map (src/Tracking.cpp:347-410) ---------------------------------------------------------
 * n trackers per call, 0 <= n <= DSDTM_LOCALMAP_MAX_DESCS; n == 0: DSDTM_OK, nothing done. Synchronous: one upload (poses and INDICES,
 * no positions), a gather launch that builds on the device what dsdtm_need_keyframes uploads, the decision kernel of
 * libdsdtm_amd_keyframe.so (keyframe.hip, linked as it is), one read-back of n verdicts, one wait. Rules K1-K4, `undefined` and the
 * verdict are those of include/dsdtm_amd_keyframe.h, unchanged.
 * Desc: map; T_cur_w (12 doubles, the frame's pose); n_valid (Get_VaildMpNums()); cur_point[n_cur_points] (HOST): the frame's map
 *   points as MAP indices in feature order, features without a point omitted, n_cur_points <= DSDTM_KF_MAX_POINTS; kf: the last
 *   keyframe's MAP index — its pose is the map's pose, its point list is its slots in slot order with point_of_slot >= 0 (whether
 *   the slot observes or not: mvFeatures[i]->Mpt is what the reference walks), positions and bad flags are read from the map;
 *   local_kf[n_local_kf] (HOST): mvpLocalKeyFrames as MAP keyframe indices, n_local_kf <= DSDTM_KF_MAX_LOCAL_KF.
 * WHY THE SLOT WALK IS THE WALK OVER mvFeatures[i]->Mpt: a slot is -1 only when the feature never had a point, or when its point went
 *   bad through rule T3 above or through rule C2 of the local-BA commit (SetBadFlag nulls the observers); the reference's feature would
 *   still hold that bad point, but K2 (:365) and Get_SceneDepth skip bad points, so leaving it out changes nothing.
 * Camera centres: Get_CameraCnt of a local keyframe is computed on the device from the map's pose [R|t] as
 *   c_i = -((R_0i * t_0 + R_1i * t_1) + R_2i * t_2), separate multiplies and adds, no fused multiply-add; gather_keyframe_desc_host
 *   (dsdtm_amd/host/dsdtm_slam_host.hpp; compile with -ffp-contract=off) and the restatement use the same formula.
 * Parity: the verdict is byte-equal to dsdtm_need_keyframes fed with the host-gathered arrays and those centres.
 * Positions are finite: dsdtm_slam_points_write refuses any that is not, so the gather does not check them again.
 * All or nothing: checked on the host before anything is enqueued, DSDTM_ERR_INVALID naming the tracker and the field, verdicts
 *   untouched (as they are when a HIP call fails) — a NULL argument, a map of another context, a point or keyframe index outside the
 *   map, a pose entry that is not finite, a count over its limit, px_samples outside 1..64. */
typedef struct dsdtm_slam_keyframe_desc {
    const dsdtm_trackmap* map;
    const double* T_cur_w;
    int32_t n_valid, n_cur_points;
    const int32_t* cur_point;
    int32_t kf, n_local_kf;
    const int32_t* local_kf;
} dsdtm_slam_keyframe_desc;
int dsdtm_slam_need_keyframes(dsdtm_slam_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* params, int n,
                              const dsdtm_slam_keyframe_desc* descs, dsdtm_keyframe_verdict* verdicts);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_SLAM_H */
