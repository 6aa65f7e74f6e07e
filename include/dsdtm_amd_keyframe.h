/*
 * dsdtm_amd_keyframe.h — C ABI of libdsdtm_amd_keyframe.so: Tracking::NeedKeyframe for n trackers on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own: the surface of
 * libdsdtm_amd.so (include/dsdtm_amd.h) is a drop-in boundary that stays exactly what it is, symbol for symbol. The add-on shares
 * the conventions of that header — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions,
 * no globals, no environment, one context per calling thread, NO CPU fallback — and its dsdtm_camera. Nothing else is shared:
 * a dsdtm_keyframe_ctx owns its own stream and staging block, so the two libraries can be used from one thread in any order.
 */
#ifndef DSDTM_AMD_KEYFRAME_H
#define DSDTM_AMD_KEYFRAME_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_keyframe_ctx dsdtm_keyframe_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_keyframe_create(int device, dsdtm_keyframe_ctx** out);
void dsdtm_keyframe_destroy(dsdtm_keyframe_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_keyframe_create when ctx == NULL). */
const char* dsdtm_keyframe_last_error(const dsdtm_keyframe_ctx* ctx);

/* ---- Tracking::NeedKeyframe ------------------------------------------------------------------------------------------
 * Replaces: bool Tracking::NeedKeyframe() (src/Tracking.cpp:347-410), the step Track_RGBDCam runs on every tracked frame after
 *           PoseOptimization, for n independent trackers in ONE submission (one upload, one launch, one read-back, one wait).
 * Poses are [R|t], 12 doubles row-major, world -> camera; T * P is R P + t row by row, as Frame::World2Pixel's callers see it.
 * "Median" is utils::GetMedian (include/Utils.h:34-40): nth_element at begin + floor(size / 2), i.e. the element at index
 * floor(m / 2) of the ascending order — for an even m the UPPER middle, never a mean.
 * All four rules are evaluated for every tracker, in the reference's order:
 *   K1 count (:352-357)        min_valid <= n_valid <= max_valid (30, 50); n_valid = Frame::Get_VaildMpNums() of the current frame.
 *   K2 pixel displacement (:359-381)  the last keyframe's map points in feature order (features without a map point are not in
 *      the list; bad ones are skipped :365); per point |World2Pixel_cur(P) - World2Pixel_kf(P)| (src/Frame.cpp:318-323,
 *      src/Keyframe.cpp:64-69, Camera::Camera2Pixel src/Camera.cpp:167-171: float intrinsics promoted to double,
 *      fx * x / z + cx, no test on z); the walk stops once the list holds px_samples entries — 31, not 30: the reference breaks on
 *      size() > 30 AFTER the push (:374). Fires when the median is > min_px_median (40, strict :378). An empty list (the
 *      reference dereferences end() there) skips the rule: n_px = 0.
 *   K3 parallax (:383-390)     D = T_kf^-1 * T_cur composed as Sophus does (unit quaternion + translation); rot = |SO3::log(D)|
 *      (the atan form), trans = |D.translation()|. Fires when rot >= min_rot || trans >= min_trans (KeyFrame.min_rot / min_trans).
 *   K4 scene depth (:392-402)  Frame::Get_SceneDepth (src/Frame.cpp:243-275) over the current frame's non-bad map points:
 *      z_i = (T_cur * P_i).z, min_depth = min z_i, median_depth = their median m. No point (the reference reads uninitialised
 *      doubles) skips the rule: n_depth = 0. For each local keyframe in order, c = T_cur * Get_CameraCnt(): fires when
 *      c.x / m >= m && c.y / m >= 0.8 m && c.z / m >= 1.3 m. NO absolute value: the reference writes fabs(a >= b), and fabs of a
 *      boolean is the boolean (:398-400). svo_kf = the first local keyframe that fires, or -1.
 * undefined = 1 when a pixel distance of K2 or a depth of K4 is not finite (a point at z = 0 of either camera: nth_element on
 * NaN is undefined in the reference): the other fields of that verdict are unspecified; the call succeeds and every other
 * tracker of the batch is unaffected.
 * Limits per tracker: n_cur_points, n_kf_points <= DSDTM_KF_MAX_POINTS; n_local_kf <= DSDTM_KF_MAX_LOCAL_KF; 1 <= px_samples <= 64;
 * 0 <= n <= DSDTM_TRACK_FRAMES_MAX (n == 0: DSDTM_OK, nothing done). All or nothing: everything is checked on the host before
 * anything is enqueued — a NULL pointer with a non-zero count, a count over its limit, px_samples out of range, a pose entry,
 * world point or camera centre that is not finite return DSDTM_ERR_INVALID naming the tracker and the field, and the verdicts
 * are left untouched (as they are when a HIP call fails). Synchronous. dsdtm_need_keyframe is the batch entry with n = 1.
 * For ONE tracker the plain host evaluation (dsdtm_host.hpp: need_keyframe_host) is the faster path; see README. */
#define DSDTM_KF_MAX_POINTS 4096
#define DSDTM_KF_MAX_LOCAL_KF 64
typedef struct dsdtm_keyframe_params {
    int32_t min_valid, max_valid;   /* 30, 50 (:354) */
    int32_t px_samples;             /* 31 (:374) */
    int32_t reserved;
    double min_px_median;           /* 40.0 (:378) */
    double min_rot, min_trans;      /* KeyFrame.min_rot, KeyFrame.min_trans (src/Tracking.cpp:26-27) */
} dsdtm_keyframe_params;
typedef struct dsdtm_keyframe_desc {
    const double* T_cur_w; const double* T_kf_w;    /* 12 each: mCurrentFrame->Get_Pose(), mpLastKF->Get_Pose() */
    int32_t n_valid;                                /* mCurrentFrame->Get_VaildMpNums() */
    int32_t n_cur_points; const double* cur_p_world; const uint8_t* cur_bad;   /* the current frame's map points (n x 3), IsBad() (NULL = none bad) */
    int32_t n_kf_points;  const double* kf_p_world;  const uint8_t* kf_bad;    /* the last keyframe's, in mvFeatures order */
    int32_t n_local_kf;   const double* local_kf_centre;                       /* n x 3: mvpLocalKeyFrames[i]->Get_CameraCnt() */
} dsdtm_keyframe_desc;
typedef struct dsdtm_keyframe_verdict {
    int32_t need;          /* 0 / 1: NeedKeyframe()'s return value */
    int32_t reason;        /* the first rule that fires, 1..4 = K1..K4 (where the reference returns); 0 = none */
    int32_t rule_mask;     /* bit i - 1 set: rule K_i fires */
    int32_t undefined;     /* 1: a non-finite pixel distance or depth; the other fields are unspecified */
    int32_t n_px, n_depth; /* samples of K2's list / of Get_SceneDepth's */
    int32_t svo_kf;        /* K4: index of the first local keyframe that fires, or -1 */
    int32_t reserved;
    double median_px;      /* 0 when n_px == 0 */
    double rot, trans;
    double min_depth, median_depth;   /* 0 when n_depth == 0 */
} dsdtm_keyframe_verdict;
int dsdtm_need_keyframe(dsdtm_keyframe_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* params,
                        const dsdtm_keyframe_desc* desc, dsdtm_keyframe_verdict* verdict);
int dsdtm_need_keyframes(dsdtm_keyframe_ctx* ctx, const dsdtm_camera* cam, const dsdtm_keyframe_params* params, int n,
                         const dsdtm_keyframe_desc* descs, dsdtm_keyframe_verdict* verdicts);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_KEYFRAME_H */
