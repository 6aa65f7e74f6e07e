/*
 * dsdtm_amd_newkf.h — C ABI of libdsdtm_amd_newkf.so: the walk and the lift of Tracking::CraeteKeyframe (src/Tracking.cpp:412-464)
 * and Tracking::CreateInitialMapRGBD (:147-196) for n trackers on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, with a header, a context and a version script of its own (see dsdtm_amd_keyframe.h for
 * what the add-ons share with include/dsdtm_amd.h: POD arguments, caller-owned memory, `int` status returns, no globals, no
 * environment, one context per calling thread, NO CPU fallback, and dsdtm_camera). A dsdtm_newkf_ctx owns its own stream and staging.
 *
 * The entry starts at the per-cell corners that dsdtm_detect_cells / dsdtm_detect_cells_frame / dsdtm_detect_cells_batch_device
 * write (the image work of Feature_detector::detect, src/Feature_detection.cpp:74-108, stays there) and ends at the columns that
 * dsdtm_trackmap_keyframe_add / dsdtm_mapping_keyframe_add and dsdtm_*_points_write take.
 */
#ifndef DSDTM_AMD_NEWKF_H
#define DSDTM_AMD_NEWKF_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_newkf_ctx dsdtm_newkf_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_newkf_create(int device, dsdtm_newkf_ctx** out);
void dsdtm_newkf_destroy(dsdtm_newkf_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_newkf_create when ctx == NULL). */
const char* dsdtm_newkf_last_error(const dsdtm_newkf_ctx* ctx);

/* ---- Tracking::CraeteKeyframe: the order-dependent rest of detect(), then the keyframe's slots ------------------------------------
 * Replaces, for n independent trackers in ONE submission (one upload, one launch, one read-back, one wait): the part of
 *   Feature_detector::detect behind the image work (src/Feature_detection.cpp:110-153) with Frame::Set_Mask (src/Frame.cpp:286-298),
 *   Frame::Add_Feature's pixel / level / bearing for the new features, and the loop of CraeteKeyframe (src/Tracking.cpp:424-455) /
 *   CreateInitialMapRGBD (:156-176), which gives every feature of the frame a map point: the one it has, or a new one lifted from depth.
 * The rules, each with its reference line (src/Feature_detection.cpp unless another file is named):
 *   K1 (:71-72)  n_existing >= max_fts: detect() returns before anything; n_new = 0. (K6 still runs over the existing features.)
 *   K2 (:110, include/Feature_detection.h:29-32)  corners are ordered by descending score. Corners of EQUAL score keep their cell
 *      index order: this project's definition (as dsdtm_amd/feature_detection.py); std::sort leaves it open. A NaN score never
 *      satisfies score > score_floor: it is dropped before the order is made.
 *   K3 (:119-122, src/Frame.cpp:286-298)  the mask, evaluated without being painted. ONLY when n_existing > 0 a pixel is masked by
 *      (a) the filled cv::circle of radius min_dist around (cvRound(px.x), cvRound(px.y)) of every existing feature with has_point
 *      (the cv::Point2f is narrowed to float before it is rounded), and (b) dyn_mask[y, x] > 200 (the threshold and
 *      the saturating subtraction of :294-296). With n_existing == 0 Set_Mask is not called: the dynamic mask is IGNORED on an empty
 *      frame. That quirk is kept. The disc is OpenCV's midpoint-span disc (drawing.cpp Circle(), filled), not a distance test: one
 *      half-width per |dy|, built once per radius; a pixel is covered when |dy| <= r and |dx| <= hw[|dy|].
 *   K4 (:124-150)  the walk, in K2's order: a corner with score > score_floor whose pixel is not masked is accepted; an accepted
 *      corner masks the disc of radius cell_size around it for every LATER corner; the walk stops after the acceptance that makes
 *      n_existing + accepted >= max_fts. A corner whose pixel lies outside the image is skipped (the reference indexes the cv::Mat
 *      unchecked there); so is a corner whose level is outside 0..15.
 *   K5 (:145, src/Frame.cpp:139-149)  a new feature has px = ((float)x, (float)y), level = the cell's level, bearing =
 *      Camera::Pixel2Camera(cv::Point2f, 1.0) computed in float and normalised in double (the formula of Frame::Add_Feature, as
 *      track.hip evaluates it). cv::undistortPoints (Frame::UndistortFeatures, src/Tracking.cpp:417) is NOT restated: OpenCV is not
 *      available to this project. The entry is defined for RECTIFIED images, where the reference's call is the identity up to
 *      rounding; that parity is unpinned.
 *   K6 (src/Tracking.cpp:424-455)  slot i of the keyframe is feature i of the frame (the existing ones, then the new ones).
 *      initial[i] set: point_of_slot = point_index[i], observes = 1, depth_of_slot = -1 (no lift). Otherwise (an existing non-initial
 *      feature, or a new one) the feature is lifted through Frame::Get_FeatureDetph(cv::Point2f) and Frame::UnProject exactly as
 *      dsdtm_frame_lift documents them: x = cvRound(px.x), y = cvRound(px.y); the depth there, or if it is 0 the first non-zero of
 *      the neighbours (-1,0), (0,-1), (1,0), (0,1) in that order, or -1; a pixel or neighbour outside the image has no depth;
 *      Pixel2Camera in float; then R^T p + (-(R^T t)) in double. z < 0: point_of_slot = -1, observes = 0. Any other z makes a new
 *      point: its index is first_point_index + its rank among the new points in slot order, observes = 1.
 * Refused before anything is enqueued, with DSDTM_ERR_INVALID naming the tracker and the field and with the results untouched (as
 * they are when a HIP call fails): a NULL array with a non-zero count; a pose entry or existing pixel that is not finite; an existing
 * feature's level outside 0..15; an initial feature with point_index < 0; a cell pixel or cell level that is negative, for cells in
 * HOST memory (cells in device memory cannot be checked: the kernel skips a bad one as K4 skips an outside pixel); capacities below
 * n_existing; n_existing outside 0..DSDTM_NEWKF_MAX_EXISTING; an array in another device's memory; params out of range.
 * Memory: the cell arrays, the depth image and the dynamic mask may EACH lie in host or in this device's memory. The kind is found
 * once per pointer (hipPointerGetAttributes): a pageable host array is copied into the context's pinned block and uploaded; a pinned
 * host array (hipHostMalloc / hipHostRegister) and a device array are read where they are. Everything else is host memory.
 * Every result of a batch is bit-equal to its single call. Synchronous. dsdtm_newkf_make is the batch entry with n = 1.
 * OUT OF SCOPE: reading the depth map of a prefetched dsdtm_frame (that needs a new symbol in libdsdtm_amd.so: the caller passes
 * its depth image again); the image work of detect(); undistortion; writing the keyframe into the resident map device to device
 * (the caller passes the columns to keyframe_add / points_write). */
#define DSDTM_NEWKF_MAX_TRACKERS 1024
#define DSDTM_NEWKF_MAX_CELLS 4096
#define DSDTM_NEWKF_MAX_EXISTING 4096
#define DSDTM_NEWKF_MAX_RADIUS 127
#define DSDTM_NEWKF_MAX_SIDE 16384
typedef struct dsdtm_newkf_params {
    int32_t width, height;          /* level-0 image; 1..DSDTM_NEWKF_MAX_SIDE */
    int32_t cell_size;              /* Camera.CellSize: the radius of K4's disc; 0..127 */
    int32_t grid_cols, grid_rows;   /* G = cols * rows <= DSDTM_NEWKF_MAX_CELLS */
    int32_t max_fts;                /* Camera.Max_fts */
    int32_t min_dist;               /* Camera.Min_dist: the radius of K3's disc; 0..127 */
    float score_floor;              /* the literal 20 of :128; finite, >= 0 */
} dsdtm_newkf_params;
typedef struct dsdtm_newkf_desc {
    /* the cells, G entries each, as dsdtm_detect_cells* writes them; host or device memory, each on its own */
    const float* cell_score; const int32_t* cell_x; const int32_t* cell_y; const int32_t* cell_level;
    /* the frame's features before detect(); host memory */
    int32_t n_existing;
    int32_t first_point_index;      /* the map's point count: new points are numbered from it; >= 0 */
    const float* px_xy;             /* n_existing x 2 */
    const int32_t* level;           /* n_existing */
    const double* bearing;          /* n_existing x 3 */
    const uint8_t* has_point;       /* mvMapPoints[k] != NULL, what Set_Mask reads (src/Frame.cpp:290) */
    const uint8_t* initial;         /* Feature::mbInitial, what CraeteKeyframe reads (src/Tracking.cpp:428) */
    const int32_t* point_index;     /* the feature's map point as an index of the resident map, or -1 */
    /* the depth image, with the meaning of dsdtm_frame_image: u16, kept as d * (1.0f / depth_scale); stride in ELEMENTS; host or device */
    const uint16_t* depth; int32_t depth_stride; float depth_scale;
    /* Frame::mDynamicMask, u8, level-0 size, stride in bytes, or NULL; host or device */
    int32_t dyn_stride; const uint8_t* dyn_mask;
    const double* T_c2w;            /* 12: mCurrentFrame->Get_Pose(), [R|t] row-major, world -> camera */
    int32_t slot_capacity;          /* entries of the six slot columns of the result */
    int32_t point_capacity;         /* points of new_p_world */
    int32_t bad_capacity;           /* entries of new_bad (ignored when new_bad is NULL) */
    int32_t reserved;
} dsdtm_newkf_desc;
typedef struct dsdtm_newkf_result {
    int32_t n_new;                  /* features added by the walk */
    int32_t n_slots;                /* n_existing + n_new */
    int32_t n_new_points;
    int32_t overflow;               /* 1: n_slots or n_new_points did not fit its capacity; the counts are right, NOTHING else of this tracker may be used */
    /* host arrays of the caller; the first five in the layout keyframe_add takes */
    int32_t* point_of_slot; uint8_t* observes; float* px_xy; int32_t* level; double* bearing;
    float* depth_of_slot;           /* the depth the lift found, -1 where it found none or no lift took place */
    double* new_p_world;            /* n_new_points x 3, in slot order: what points_write(first = first_point_index, ...) takes */
    uint8_t* new_bad;               /* n_new_points zeros (points_write's `bad`), or NULL */
} dsdtm_newkf_result;
int dsdtm_newkf_make(dsdtm_newkf_ctx* ctx, const dsdtm_camera* cam, const dsdtm_newkf_params* params, const dsdtm_newkf_desc* desc,
                     dsdtm_newkf_result* result);
int dsdtm_newkf_make_batch(dsdtm_newkf_ctx* ctx, const dsdtm_camera* cam, const dsdtm_newkf_params* params, int n,
                           const dsdtm_newkf_desc* descs, dsdtm_newkf_result* results);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_NEWKF_H */
