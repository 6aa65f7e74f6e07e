/*
 * dsdtm_amd_motion.h — C ABI of libdsdtm_amd_motion.so: the moving-object mask of Tracking::MotionRemoval (fastMCD) on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, like libdsdtm_amd_keyframe.so: a header, a context and sources of its own, so that the
 * surface of libdsdtm_amd.so (include/dsdtm_amd.h) stays exactly what it is. It shares that header's conventions — POD arguments,
 * caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling
 * thread, NO CPU fallback — and nothing else: a dsdtm_motion_ctx owns its own stream and staging block.
 *
 * Replaces: Moving_Detecter::Mod_FastMCD (src/Moving_Detection.cpp:19-34) = MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137)
 *           up to and including BGModel.update(detect_img) (:92): the 5x5 median of the image (cvSmooth(CV_MEDIAN, 5), :88: the median of
 *           25 bytes, BORDER_REPLICATE), ProbModel::motionCompensate (Thirdparty/fastMCD/include/prob_model.h:169-371) and
 *           ProbModel::update (:373-582); and the test Frame::Motion_Removal makes per feature (src/Frame.cpp:342-363, the test :352).
 *           Tracking::MotionRemoval (src/Tracking.cpp:487-512) calls these on every tracked frame — in the reference as it stands that
 *           call is COMMENTED OUT (src/Tracking.cpp:230), so this is the stage the reference's authors wrote, not one it runs.
 * OUT OF SCOPE: cv::findHomography and its RANSAC (the caller's; H is an argument); the contour step of MCDWrapper::Run (:98-128: the
 *           bounding rectangle of the largest contourArea contour filled into the mask — `mask` here is detect_img BEFORE it; the
 *           whole Run, that step included, is libdsdtm_amd_mcd.so's, include/dsdtm_amd_mcd.h); KLTWrapper (initialised at :75, never used on this path);
 *           Moving_Detecter::Mod_FrameDiff; dsdtm_track_frame, which is unchanged and knows nothing of this library.
 */
#ifndef DSDTM_AMD_MOTION_H
#define DSDTM_AMD_MOTION_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdtm_motion_ctx dsdtm_motion_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_motion_create(int device, dsdtm_motion_ctx** out);
/* Models of the context must be destroyed first. */
void dsdtm_motion_destroy(dsdtm_motion_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_motion_create when ctx == NULL). */
const char* dsdtm_motion_last_error(const dsdtm_motion_ctx* ctx);

/* ---- the model ----------------------------------------------------------------------------------------------------------
 * A dsdtm_motion_model is the device-resident state of one ProbModel (one tracker) for width x height images: a grid of
 * floor(width / 4) x floor(height / 4) cells (BLOCK_SIZE 4, params.h:25) and the twelve float arrays m_Mean, m_Var, m_Age,
 * m_Mean_Temp, m_Var_Temp, m_Age_Temp, each x 2 modes (NUM_MODELS). DSDTM_MOTION_MIN_SIDE <= width, height <= DSDTM_MOTION_MAX_SIDE;
 * neither needs to be a multiple of 4 (the last width % 4 columns and height % 4 rows belong to no cell, as in the reference).
 * The device keeps TWO generations of the arrays and a step writes the one it does not read: compensation of a cell gathers
 * m_Mean / m_Var / m_Age of its neighbours as they were BEFORE the step while update overwrites them, and a step that fails leaves
 * the model as it was.
 * Creation and dsdtm_motion_model_reset perform ProbModel::init (prob_model.h:121-167): all SIX arrays zero, then
 * motionCompensate(identity) + update(NULL) on an all-zero image. The reference runs init on a cvCreateImage buffer nobody has
 * written yet (MCDWrapper.cpp:69-73; the median comes at :88) and leaves the _Temp arrays of `new float[]` unset (:142-144); in
 * practice both are fresh zero pages. ZEROS ARE THIS PROJECT'S DEFINITION of both.
 * dsdtm_motion_model_read / _write move the state to / from the host: 12 * cells floats, the arrays in the order above, mode 0 before
 * mode 1 within each, cell (i, j) at i + j * floor(width / 4). They serve checkpointing and tests. Synchronous. */
#define DSDTM_MOTION_MIN_SIDE 16
#define DSDTM_MOTION_MAX_SIDE 4096
#define DSDTM_MOTION_MAX_FEATURES 16384
#define DSDTM_MOTION_STEPS_MAX 1024
typedef struct dsdtm_motion_model dsdtm_motion_model;
int dsdtm_motion_model_create(dsdtm_motion_ctx* ctx, int width, int height, dsdtm_motion_model** out);
void dsdtm_motion_model_destroy(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model);
int dsdtm_motion_model_reset(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model);
int dsdtm_motion_model_read(dsdtm_motion_ctx* ctx, const dsdtm_motion_model* model, float* out);
int dsdtm_motion_model_write(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model, const float* in);

/* ---- one step -----------------------------------------------------------------------------------------------------------
 * One MCDWrapper::Run up to BGModel.update(detect_img), in one submission (one upload, the launch, one read-back) and one wait.
 *   image        8-bit single channel, width x height of the model, rows `stride` bytes apart (stride >= width), in ordinary or pinned
 *                host memory (copied into the upload) or in this device's memory (read where it is; hipPointerGetAttributes decides,
 *                as for dsdtm_track_frame's image). Another device's memory is refused.
 *   H            9 doubles, row-major: what the caller got from cv::findHomography(tPointsA, tPointsB, CV_RANSAC)
 *                (src/Moving_Detection.cpp:28-31). It maps a cell centre of the current frame to where its model lies (prob_model.h:189-191).
 *   mask         host memory, rows mask_stride >= width apart; NULL = not wanted. Receives detect_img: 255 / 0 per pixel; rows and
 *                columns beyond 4 * the model grid are 0 (cvSet :377). Bytes of a row beyond `width` are not touched.
 *   feature_px   n_features x 2 floats (x, y), 0 <= n_features <= DSDTM_MOTION_MAX_FEATURES; feature_on_mask[i] = 1 when the mask at
 *                (cvRound(x), cvRound(y)) is 255, else 0 — the test of Frame::Motion_Removal (src/Frame.cpp:352), made on the device against
 *                the mask where it lies (so `mask` may be NULL). cvRound rounds to nearest, HALVES TO EVEN, as cv::Mat::at(Point2f -> Point)
 *                does. A feature that is not finite or rounds outside the image returns DSDTM_ERR_INVALID naming it (the reference reads
 *                out of bounds there).
 * Traps of the reference that are kept (prob_model.h): the _Temp arrays PERSIST across steps — where all four source cells are off the
 * model (sumW == 0, :277, :341) m_Mean_Temp keeps what the previous step left, "oldest to 0" block included (:430-439), and update uses
 * it (:494, :505), var and age being forced at :357-361; "Make Oldest Idx to 0" is not a swap (>= against 0: equal ages pick mode 1;
 * mode 0 receives mode 1; mode 1 becomes (cur_mean, INIT_BG_VAR, 0)); MIN_BG_VAR (900) is larger than INIT_BG_VAR (225); the mask uses
 * m_Mean[0] AFTER this step's update but m_Var_Temp[0] and m_Age_Temp[0] > 1 from before it (:542-546).
 * Arithmetic: the reference's types as compiled with -std=c++11 — float variables and array elements; a right-hand side with a double
 * literal or h[] in it evaluated in double and rounded once at the assignment; pow(float, (int)2) the exact double product; the
 * comparisons against 2.0 * var in double; exp the double one — in the reference's order, without contraction. Only exp can differ
 * from a host libm, in its last place, and only in cells whose compensated variance exceeds VAR_MIN_NOISE_T (2500).
 * Host validation (DSDTM_ERR_INVALID, naming the field; everything is checked before anything is enqueued): NULL ctx / model / image /
 * H; a model of another context; stride < width; mask_stride < width; n_features out of range or its arrays NULL; H not finite;
 * h6 * X + h7 * Y + h8 (evaluated as :189 does, rounded to float) not > 0 at the centres (X, Y) = (4 i + 2, 4 j + 2) of the four corner
 * cells — the denominator is linear, so it is then positive at every cell; the reference divides by it unchecked.
 * On the device a transformed cell index floor(newI), floor(newJ) (:197-198) of magnitude 2^30 or more is treated as OFF THE MODEL
 * (that cell has sumW == 0 and takes the border branch :357); the reference's float -> int conversion is undefined there.
 * All or nothing: after any failure the outputs are untouched and the model is as it was. */
int dsdtm_motion_step(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model, const uint8_t* image, int stride, const double* H,
                      uint8_t* mask, int mask_stride, int n_features, const float* feature_px, uint8_t* feature_on_mask);

/* ---- n independent models in ONE submission -------------------------------------------------------------------------------
 * The same step for n models (0 <= n <= DSDTM_MOTION_STEPS_MAX; n == 0: DSDTM_OK, nothing done), each with its own size, image, H and
 * outputs: one upload, ONE launch of the step kernel (the model is the grid's third dimension) and one of the feature lookup, one
 * read-back, one wait. Each result is bit-equal to its single dsdtm_motion_step. All or nothing: every argument of every desc is
 * checked on the host before anything is enqueued and a failure names the index and the field; the same model twice is an error. */
typedef struct dsdtm_motion_desc {
    dsdtm_motion_model* model;
    const uint8_t* image; int32_t stride;
    int32_t mask_stride; uint8_t* mask;
    const double* H;
    int32_t n_features; int32_t reserved;
    const float* feature_px; uint8_t* feature_on_mask;
} dsdtm_motion_desc;
int dsdtm_motion_steps(dsdtm_motion_ctx* ctx, int n, const dsdtm_motion_desc* descs);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_MOTION_H */
