/*
 * dsdtm_amd_trackmap.h — C ABI of libdsdtm_amd_trackmap.so: the local-map columns of dsdtm_track_desc (include/dsdtm_amd.h: mp_world,
 * mp_found, mp_bad, obs_offset, obs_kf, obs_px, obs_level, obs_bearing) from a map that is RESIDENT on the MI355X (gfx950), for n trackers
 * per call. The call runs the selection of dsdtm_localmap_select (include/dsdtm_amd_localmap.h, rules L1-L4) and then flattens the
 * selected points with their observations on the device: the walk over MapPoint / KeyFrame objects a caller otherwise does per frame.
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own; the conventions are those of the
 * other add-on headers — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no
 * environment, one context per calling thread, NO CPU fallback. It holds a SUPERSET of the map of libdsdtm_amd_localmap.so: a tracker
 * that feeds dsdtm_track_frame(s) keeps ONE resident map, this one; libdsdtm_amd_localmap.so remains for callers who want the lists
 * alone. The plain host evaluation of the same rules is select_local_map_host + flatten_local_map_host
 * (dsdtm_amd/host/dsdtm_trackmap_host.hpp), which needs no library.
 */
#ifndef DSDTM_AMD_TRACKMAP_H
#define DSDTM_AMD_TRACKMAP_H

#include "dsdtm_amd_localmap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_trackmap_ctx dsdtm_trackmap_ctx;
typedef struct dsdtm_trackmap dsdtm_trackmap;         /* one tracker's (or one rig's) map, resident on the device */

/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_trackmap_create(int device, dsdtm_trackmap_ctx** out);
/* Maps that are still alive are released with the context. */
void dsdtm_trackmap_destroy(dsdtm_trackmap_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_trackmap_create when ctx == NULL). */
const char* dsdtm_trackmap_last_error(const dsdtm_trackmap_ctx* ctx);

/* ---- the resident map ----------------------------------------------------------------------------------------------
 * Indices and limits are those of include/dsdtm_amd_localmap.h (DSDTM_LOCALMAP_MAX_POINTS, _MAX_KEYFRAMES, _MAX_SLOTS per keyframe);
 * points and keyframes are numbered in the order they were added and never removed.
 *   per point     the position (MapPoint::Get_Pose(), 3 doubles), IsBad(), Get_FoundNums() as int32;
 *   per keyframe  the pose (KeyFrame::Get_Pose(), [R|t], 12 doubles row-major, world -> camera) and, per slot (one per feature of
 *                 mvFeatures): point_of_slot (KeyFrame::mvMapPoints as a point index, -1 = NULL), observes (0 / 1) and the observing
 *                 feature: Feature::mpx (2 floats), mlevel (int32), mNormal (3 doubles).
 * SLOTS ARE NOT OBSERVATIONS. observes[s] == 1 means "mObservations of point point_of_slot[s] holds (this keyframe, s)". The two
 * differ in the reference: Optimizer::LocalBundleAdjustment's outlier pass (src/Optimizer.cpp:266-267) erases the observation first
 * (MapPoint::Erase_Observation), after which KeyFrame::Erase_MapPointMatch(MapPoint*) finds no index and leaves mvMapPoints pointing
 * at the point: such a slot still lists the point for rule L4 and is written with observes = 0.
 * THE CALLER'S DUTY: MapPoint::Add_Observation (src/MapPoint.cpp:45-55) keeps at most one entry per keyframe, so no two observing
 * slots of one keyframe may name the same point. Nothing checks it, and nothing is undefined when it is violated: EVERY observing slot
 * is emitted as one observation, in slot order.
 * The UPDATES copy the caller's arrays into the context's pinned block and enqueue the upload before they return: the caller's
 * buffers are free at once, and the update holds for every later call on that context, in call order. Everything is checked on the
 * host before anything is enqueued; a failed update — DSDTM_ERR_INVALID naming the field, or a failed HIP call — leaves the map as it
 * was. Device arrays grow geometrically. */
int dsdtm_trackmap_map_create(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap** out);
void dsdtm_trackmap_map_destroy(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap* map);

/* Points [first, first + n): first == the current count appends, below it rewrites (MapPoint::Set_Pose after local BA, SetBadFlag), a
 * gap is refused. bad (n flags) and found (n counts) may each be NULL: zeros for appended points, unchanged for rewritten ones. */
int dsdtm_trackmap_points_write(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap* map, int first, int n, const double* p_world, const uint8_t* bad,
                                const int32_t* found);
/* A scattered update of the found counts: found count of point index[i] = found[i] — what a tracked frame's <= 256 matches change
 * through MapPoint::IncreaseFound / EraseFound. An index outside the map's points and an index that occurs twice in the call are refused. */
int dsdtm_trackmap_found_write(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap* map, int n, const int32_t* index, const int32_t* found);
/* A new keyframe (Tracking::CraeteKeyframe): its pose and its n_slots slots (0 <= n_slots <= DSDTM_LOCALMAP_MAX_SLOTS): point_of_slot
 * (-1 or a point index below the point count), observes (0 / 1; 1 on a -1 slot is refused), px_xy (2 floats per slot), level, bearing (3
 * doubles per slot). The slot count and the feature columns are fixed from here on (mvFeatures of a keyframe does not change).
 * *out_index (may be NULL): the keyframe's index. */
int dsdtm_trackmap_keyframe_add(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                                const uint8_t* observes, const float* px_xy, const int32_t* level, const double* bearing, int* out_index);
/* An existing keyframe: a new pose (NULL = keep; KeyFrame::Set_Pose after local BA) and / or its slots [first_slot, first_slot + n)
 * with their flags (KeyFrame::Add_MapPoint + MapPoint::Add_Observation, Erase_MapPointMatch, MapPoint::Erase_Observation;
 * first_slot + n <= the keyframe's slot count; n == 0: the pose alone). Pose, slots and flags change together or not at all. */
int dsdtm_trackmap_keyframe_write(dsdtm_trackmap_ctx* ctx, dsdtm_trackmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                                  const int32_t* point_of_slot, const uint8_t* observes);
/* The whole map back to the host, for checkpointing and tests; synchronous. The counts are always written. The arrays are filled
 * (complete = 1) when every capacity covers its count (an array whose count is 0 may be NULL); otherwise nothing but the counts is
 * written (complete = 0) and the call still returns DSDTM_OK: call once with capacities of 0 to size the arrays. */
typedef struct dsdtm_trackmap_image {
    int32_t n_points, n_keyframes;                 /* out */
    int64_t n_slots_total;                         /* out: the sum of the keyframes' slot counts */
    int32_t complete, reserved;                    /* out */
    int32_t point_capacity, keyframe_capacity;     /* in: elements the arrays below hold */
    int64_t slot_capacity;                         /* in */
    double* p_world; uint8_t* bad; int32_t* found; /* point_capacity x 3, point_capacity, point_capacity */
    double* T_kf_w; int32_t* n_slots; int64_t* slot_offset;   /* keyframe_capacity x 12, keyframe_capacity, keyframe_capacity */
    int32_t* point_of_slot; uint8_t* observes;     /* slot_capacity each: keyframe k's slots are [slot_offset[k], slot_offset[k] + n_slots[k]) */
    float* px_xy; int32_t* level; double* bearing; /* slot_capacity x 2, slot_capacity, slot_capacity x 3 */
} dsdtm_trackmap_image;
int dsdtm_trackmap_map_read(dsdtm_trackmap_ctx* ctx, const dsdtm_trackmap* map, dsdtm_trackmap_image* out);

/* ---- the local map of a tracked frame -----------------------------------------------------------------------------
 * Replaces: Tracking::GetCloseKeyFrames and the selection of Tracking::UpdateLocalMap (src/Tracking.cpp:258-345) AND the caller's walk
 *           that turns the selected MapPoints into dsdtm_track_desc's columns, for n descs in ONE submission: one upload (the
 *           descs as the device sees them: the poses with the maps' device arrays and the offsets of the outputs), the launches,
 *           one read-back, one wait. Synchronous.
 * Selection: kf, kf_dist, point, point_kf and n_close / n_kf / n_points are exactly what dsdtm_localmap_select returns for the same
 *   map, pose, camera and params: rules L1-L4 of include/dsdtm_amd_localmap.h (the same two launches run here); the lists are equal,
 *   kf_dist is bit-equal.
 * Columns: for the emitted points i = 0 .. m-1, m = min(n_points, point_capacity), with p = point[i]:
 *   mp_world[3i ..] the position's three doubles, mp_found[i], mp_bad[i] (always 0: L4 skips bad points; written all the same),
 *   obs_offset[0 .. m]: point i's observations are j in [obs_offset[i], obs_offset[i + 1]); obs_offset[m] = n_obs.
 *   Per observation j: obs_kf[j] (the MAP's keyframe index), obs_px[2j ..], obs_level[j], obs_bearing[3j ..]: the observing slot's
 *   feature columns. No floating-point operation happens anywhere: every value is a copy, bit for bit.
 * Observation order: point i's observations are the observing slots (observes == 1, point_of_slot == p) of ALL keyframes of the map,
 *   not only the local ones (MapPoint::Get_ClosetObs walks the whole mObservations, src/MapPoint.cpp:149-161), in ascending
 *   (keyframe index, slot index) order. That order is this project's definition (tracking.flatten_local_map: sorted(mObservations) by
 *   keyframe index): the reference iterates a std::map<KeyFrame*, ...>, whose order follows pointer values. A point with no
 *   observation has an empty segment.
 * Capacities: point_capacity <= DSDTM_TRACKMAP_MAX_LOCAL_POINTS (the limit of dsdtm_track_desc.n_points); n_points beyond it sets
 *   overflow_points and the first point_capacity points are written, complete with their observations. n_obs is the full
 *   observation count of the emitted points; n_obs > obs_capacity sets overflow_obs: the point columns are still complete and
 *   obs_offset is the full prefix sum, but only the observations j < obs_capacity are written. A result with either flag set MUST NOT
 *   be handed on to the tracker (obs_offset would address observations that were not written). The written prefix is the true prefix
 *   whatever the timing; for the one point whose observations cross obs_capacity this costs, on ONE workgroup of that desc, a scan of
 *   the map's slots per observation of that point below obs_capacity (at most its observation count times slots / 256 loads) — paid
 *   only with overflow_obs, so a caller who sizes obs_capacity from the last frame's n_obs plus a margin never pays it.
 * Hand-over: the columns go into a dsdtm_track_desc unchanged, with n_points = m, and are paired with kf = EVERY keyframe of the map
 *   in index order and T_kf_w = their poses (obs_kf indexes that list). dsdtm_track_desc allows 4096 keyframes; this call does not
 *   enforce that limit on the map.
 * Memory: a call's device and pinned blocks hold, per desc, 8 bytes per keyframe of its map, 45 bytes per point of point_capacity and
 *   48 bytes per observation of obs_capacity (40 of them come back); the read-back is sized by the CAPACITIES, so pass capacities near
 *   what is needed. A call whose blocks would exceed DSDTM_TRACKMAP_MAX_CALL_BYTES is refused (DSDTM_ERR_INVALID, the size named);
 *   nothing is clipped. A block that cannot be allocated fails with DSDTM_ERR_HIP.
 * All or nothing: checked on the host before anything is enqueued, DSDTM_ERR_INVALID naming the desc and the field, outputs
 *   untouched — a NULL argument, a map of another context, a pose entry that is not finite, n_local outside
 *   1..DSDTM_LOCALMAP_MAX_LOCAL, boundary < 0, a camera with a non-positive size, point_capacity < 0 or above the limit,
 *   obs_capacity < 0. 0 <= n <= DSDTM_LOCALMAP_MAX_DESCS; n == 0: DSDTM_OK, nothing done. Output entries behind what a result reports
 *   are left untouched. The same map may appear in several descs. */
#define DSDTM_TRACKMAP_MAX_LOCAL_POINTS 4096
#define DSDTM_TRACKMAP_MAX_CALL_BYTES 2147483648ll
typedef struct dsdtm_trackmap_desc {
    const dsdtm_trackmap* map;
    const double* T_cur_w;                  /* the frame's pose, 12 doubles */
    int32_t point_capacity, obs_capacity;
    int32_t* kf; double* kf_dist;           /* n_local each: the local keyframes, nearest first */
    int32_t* point; int32_t* point_kf;      /* point_capacity each (the arrays of point_capacity may be NULL when it is 0) */
    double* mp_world; int32_t* mp_found; uint8_t* mp_bad;      /* point_capacity x 3, point_capacity, point_capacity */
    int32_t* obs_offset;                    /* point_capacity + 1 (never NULL) */
    int32_t* obs_kf; float* obs_px; int32_t* obs_level; double* obs_bearing;   /* obs_capacity, x 2, x 1, x 3 (may be NULL when it is 0) */
} dsdtm_trackmap_desc;
typedef struct dsdtm_trackmap_result {
    int32_t n_close;          /* keyframes with a visible point */
    int32_t n_kf;             /* min(n_close, n_local) */
    int32_t n_points;         /* the full length of the local point list, also when it exceeds point_capacity */
    int32_t n_obs;            /* the observations of the emitted points, also when they exceed obs_capacity */
    int32_t overflow_points;  /* 1: n_points > point_capacity */
    int32_t overflow_obs;     /* 1: n_obs > obs_capacity */
} dsdtm_trackmap_result;
int dsdtm_trackmap_local(dsdtm_trackmap_ctx* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                         const dsdtm_trackmap_desc* descs, dsdtm_trackmap_result* results);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_TRACKMAP_H */
