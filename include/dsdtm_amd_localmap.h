/*
 * dsdtm_amd_localmap.h — C ABI of libdsdtm_amd_localmap.so: the keyframe and point selection of Tracking::UpdateLocalMap
 * (Tracking::GetCloseKeyFrames included) on a map that is RESIDENT on the MI355X (gfx950), for n trackers per call.
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own: the surface of
 * libdsdtm_amd.so (include/dsdtm_amd.h) stays exactly what it is, symbol for symbol. The add-on shares the conventions of that
 * header — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no
 * environment, one context per calling thread, NO CPU fallback — and its dsdtm_camera. Nothing else is shared: a
 * dsdtm_localmap_ctx owns its own stream and staging blocks. The plain host evaluation of the same rules is
 * select_local_map_host (dsdtm_amd/host/dsdtm_localmap_host.hpp), which needs no library.
 */
#ifndef DSDTM_AMD_LOCALMAP_H
#define DSDTM_AMD_LOCALMAP_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_localmap_ctx dsdtm_localmap_ctx;
typedef struct dsdtm_localmap dsdtm_localmap;         /* one tracker's (or one rig's) map, resident on the device */

/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_localmap_create(int device, dsdtm_localmap_ctx** out);
/* Destroy the maps of the context first (maps that are still alive are released with it). */
void dsdtm_localmap_destroy(dsdtm_localmap_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_localmap_create when ctx == NULL). */
const char* dsdtm_localmap_last_error(const dsdtm_localmap_ctx* ctx);

/* ---- the resident map ----------------------------------------------------------------------------------------------
 * A map is what Tracking::GetCloseKeyFrames and Tracking::UpdateLocalMap read of DSDTM::Map: per map point its position
 * (MapPoint::Get_Pose()) and IsBad(); per keyframe (Map::GetAllKeyFrames(), include/Map.h:60) its pose (KeyFrame::Get_Pose(),
 * [R|t], 12 doubles row-major, world -> camera) and KeyFrame::mvMapPoints as point indices, -1 for a NULL slot. Points and
 * keyframes are numbered in the order they were added; neither is ever removed (a point that leaves the map is flagged bad,
 * MapPoint::SetBadFlag; a keyframe's slots are set to -1, KeyFrame::Erase_MapPointMatch).
 * Limits (DSDTM_ERR_INVALID beyond): */
#define DSDTM_LOCALMAP_MAX_POINTS 1048576
#define DSDTM_LOCALMAP_MAX_KEYFRAMES 16384
#define DSDTM_LOCALMAP_MAX_SLOTS 4096      /* per keyframe */
#define DSDTM_LOCALMAP_MAX_LOCAL 64        /* n_local */
#define DSDTM_LOCALMAP_MAX_DESCS 1024      /* descs per dsdtm_localmap_select */
/* The three UPDATES copy the caller's arrays into the context's pinned block and enqueue the upload on the context's stream
 * before they return: the caller's buffers are free at once, and the update holds for every later call on that context, in call
 * order. Device arrays grow geometrically (a new allocation is filled by a device-to-device copy on the stream; the old one is
 * released once the stream has passed it). Everything is checked on the host before anything is enqueued, and a failed update —
 * DSDTM_ERR_INVALID naming the field, or a failed HIP call — leaves the map as it was. */
int dsdtm_localmap_map_create(dsdtm_localmap_ctx* ctx, dsdtm_localmap** out);
void dsdtm_localmap_map_destroy(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map);

/* Points [first, first + n): position (3 doubles each) and IsBad() flag (NULL = none bad). first <= the current count:
 * first == count appends, below it rewrites (MapPoint::Set_Pose after local BA, SetBadFlag), a gap is refused. n == 0: nothing. */
int dsdtm_localmap_points_write(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, int first, int n, const double* p_world, const uint8_t* bad);
/* A new keyframe: its pose and its n_slots slots (0 <= n_slots <= DSDTM_LOCALMAP_MAX_SLOTS; a slot is -1 or a point index below
 * the point count at the time of the call). The slot count is fixed from here on (mvMapPoints has one entry per feature).
 * *out_index (may be NULL): the keyframe's index. */
int dsdtm_localmap_keyframe_add(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, const double* T_kf_w, int n_slots, const int32_t* point_of_slot,
                                int* out_index);
/* An existing keyframe: a new pose (NULL = keep; KeyFrame::Set_Pose after local BA) and / or its slots [first_slot, first_slot + n)
 * (KeyFrame::Add_MapPoint, Erase_MapPointMatch; first_slot + n <= the keyframe's slot count; n == 0: the pose alone). */
int dsdtm_localmap_keyframe_write(dsdtm_localmap_ctx* ctx, dsdtm_localmap* map, int kf, const double* T_kf_w, int first_slot, int n,
                                  const int32_t* point_of_slot);
/* The whole map back to the host, for checkpointing and tests; synchronous. The counts are always written. The arrays are
 * filled (complete = 1) when every capacity covers its count (an array whose count is 0 may be NULL); otherwise nothing but
 * the counts is written (complete = 0) and the call still returns DSDTM_OK: call once with capacities of 0 to size the arrays. */
typedef struct dsdtm_localmap_image {
    int32_t n_points, n_keyframes;                 /* out */
    int64_t n_slots_total;                         /* out: the sum of the keyframes' slot counts */
    int32_t complete, reserved;                    /* out */
    int32_t point_capacity, keyframe_capacity;     /* in: elements the arrays below hold */
    int64_t slot_capacity;                         /* in */
    double* p_world; uint8_t* bad;                 /* point_capacity x 3, point_capacity */
    double* T_kf_w; int32_t* n_slots; int64_t* slot_offset;   /* keyframe_capacity x 12, keyframe_capacity, keyframe_capacity */
    int32_t* point_of_slot;                        /* slot_capacity: keyframe k's slots are [slot_offset[k], slot_offset[k] + n_slots[k]) */
} dsdtm_localmap_image;
int dsdtm_localmap_map_read(dsdtm_localmap_ctx* ctx, const dsdtm_localmap* map, dsdtm_localmap_image* out);

/* ---- the selection --------------------------------------------------------------------------------------------------
 * Replaces: Tracking::GetCloseKeyFrames (src/Tracking.cpp:315-345) and the keyframe and point selection of
 *           Tracking::UpdateLocalMap (src/Tracking.cpp:258-297), for n descs in ONE submission: one upload (the poses), two
 *           launches, one read-back, one wait. ReprojectPoint, IsinFrustum and SetReferenceMapPoints (:299-312) are not part of
 *           it: the first is in dsdtm_track_frame(s), the other two stay the caller's.
 * For one desc, with the map's K keyframes in index order:
 *   L1 visible keyframe (:320-336). Keyframe k is CLOSE when at least one of its slots holds a point index p >= 0 (:324; IsBad()
 *      is NOT looked at here, as in the reference) whose position is not exactly (+-0, +-0, +-0) (Get_Pose().isZero(0), :327) and
 *      for which Frame::isVisible passes (:330, src/Frame.cpp:300-311): Pc = R X + t, each row m0*X0 + m1*X1 + m2*X2 + m3 left to
 *      right without fused multiply-add; Pc.z < 0.0: not visible (src/Frame.cpp:303); u = (double)fx * Pc.x / Pc.z + (double)cx,
 *      v likewise (Camera::Camera2Pixel, src/Camera.cpp:167-171); Camera::IsInImage(cv::Point2f(u, v), boundary, 0)
 *      (src/Camera.cpp:187-193): cvRound of the value narrowed to float FIRST, halves to even, boundary <= x < width - boundary
 *      and the same in y. A u or v that is not finite or whose magnitude is >= 1e9 is not in the image (cvRound is undefined
 *      there; Pc.z == 0 lands here). The reference's `break` at the first visible point (:334) is an early exit: the result is an
 *      "any".
 *   L2 distance (:333). d_k = sqrt(dx*dx + (dy*dy + dz*dz)), d = t_cur - t_k: the translations of the two world -> camera poses
 *      (Get_Pose().translation()), NOT the camera centres — what the reference computes. The sum is Eigen's 3-vector
 *      reduction, p0 + (p1 + p2).
 *   L3 order (:267-268: std::list::sort, stable). The close keyframes by ascending d; equal d keeps MAP INDEX ORDER. That tie
 *      rule is this project's definition: the reference's list is filled from a std::set<KeyFrame*> (include/Map.h:60), so its
 *      ties follow pointer values. The first n_local (:277: 10) are the local keyframes.
 *   L4 local points (:277-297). Walk the local keyframes in that order and each one's slots in slot order; skip -1 slots (:288),
 *      bad points (:291) and any point already emitted in this call (mLastProjectedFrameId, :294-297): the first occurrence
 *      fixes both the position in the list and point_kf. The emitted order is the order in which the reference calls
 *      ReprojectPoint (:299), hence the order dsdtm_track_desc's points must have.
 * The output is a pure function of the map and the desc (no "first to arrive" anywhere): kf_dist is bit-equal to the host
 * evaluation, the lists are equal.
 * Outputs per desc: kf[0 .. n_kf) and kf_dist[0 .. n_kf) (entries from n_kf on are left untouched), point[] and point_kf[] up
 * to min(n_points, point_capacity) (the rest untouched). The same map may appear in several descs (select only reads it).
 * Limits: 1 <= n_local <= DSDTM_LOCALMAP_MAX_LOCAL; 0 <= point_capacity <= n_local * DSDTM_LOCALMAP_MAX_SLOTS;
 * 0 <= n <= DSDTM_LOCALMAP_MAX_DESCS (n == 0: DSDTM_OK, nothing done). All or nothing: checked on the host before anything is
 * enqueued, DSDTM_ERR_INVALID naming the desc and the field, outputs untouched — a NULL argument, a map of another context, a
 * pose entry that is not finite, a limit exceeded, n_local < 1, boundary < 0, a camera with a non-positive size. Synchronous.
 * One select is one workgroup's latency (140-190 us) whatever the map; select_local_map_host costs about 0.9 us per keyframe of 300
 * slots: for ONE pose the host function is the faster call below about 170 keyframes, this entry above; a batch of 64 or more wins
 * from 100 keyframes on (README, profiles/r17_local_map.txt). */
typedef struct dsdtm_localmap_params {
    int32_t n_local;     /* 10: src/Tracking.cpp:277 */
    int32_t boundary;    /* 0: Frame::isVisible's default, include/Frame.h:83 */
} dsdtm_localmap_params;
typedef struct dsdtm_localmap_desc {
    const dsdtm_localmap* map;
    const double* T_cur_w;                  /* the frame's pose, 12 doubles */
    int32_t* kf; double* kf_dist;           /* n_local each: the chosen keyframes, nearest first */
    int32_t point_capacity; int32_t reserved;
    int32_t* point; int32_t* point_kf;      /* point_capacity each (NULL with 0): the local points in walk order, and the position
                                               (0 .. n_kf - 1) in kf[] of the keyframe that listed it first */
} dsdtm_localmap_desc;
typedef struct dsdtm_localmap_result {
    int32_t n_close;   /* keyframes with a visible point (the length of tClose_kfs) */
    int32_t n_kf;      /* min(n_close, n_local) */
    int32_t n_points;  /* the full length of the list, also when it exceeds point_capacity */
    int32_t overflow;  /* 1: n_points > point_capacity, the first point_capacity entries were written */
} dsdtm_localmap_result;
int dsdtm_localmap_select(dsdtm_localmap_ctx* ctx, const dsdtm_camera* cam, const dsdtm_localmap_params* prm, int n,
                          const dsdtm_localmap_desc* descs, dsdtm_localmap_result* results);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_LOCALMAP_H */
