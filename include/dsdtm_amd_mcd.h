/*
 * dsdtm_amd_mcd.h — C ABI of libdsdtm_amd_mcd.so: the WHOLE of MCDWrapper::Run on the MI355X (gfx950) — the moving-object mask of
 * include/dsdtm_amd_motion.h and, behind it, the contour box that Frame::Motion_Removal actually tests features against.
 *
 * An ADD-ON library, the tenth, and a SUPERSET of libdsdtm_amd_motion.so as libdsdtm_amd_slam.so is of the mapping one: contexts and
 * models are that library's implementation (csrc/motion_api_body.h) compiled under the dsdtm_mcd_* names, motion.hip is linked as it is,
 * and the contour kernels (csrc/contour.hip) are new. A model belongs to the context that made it: a process that wants the whole Run
 * keeps its models in a dsdtm_mcd_ctx. libdsdtm_amd.so and libdsdtm_amd_motion.so are unchanged. Conventions as in dsdtm_amd_motion.h:
 * POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no globals, no environment, one context per calling
 * thread, NO CPU fallback (the host evaluation is host/dsdtm_mcd_host.hpp, which needs no library).
 *
 * Replaces: MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137) whole. Up to BGModel.update(detect_img) (:92) it is
 *           dsdtm_motion_step, statement by statement (see that header). Then (:98-128): findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) on
 *           the mask (:104), the contour with the largest contourArea (:108-118, `area > maxArea` from 0), its boundingRect (:120) filled
 *           with 255 by cv::rectangle(..., CV_FILLED) (:123), and that image returned (:126) — which Frame::Motion_Removal
 *           (src/Frame.cpp:342-363, the test :352) reads.
 * OUT OF SCOPE: KLTWrapper, Moving_Detecter::Mod_FrameDiff, cv::findHomography (include/dsdtm_amd_homography.h), masks of more than
 *           DSDTM_MCD_MAX_PIXELS pixels, OpenCV <= 3.1 (where findContours overwrites its input).
 *
 * PARITY. OpenCV is not available to this project, in source or binary. KEPT is the documented shape of OpenCV 3.2 (the version the
 * reference's CMakeLists.txt names): the source image is not modified, pixels on the image edge take part, external contours of
 * 8-connected non-zero pixels by Suzuki's border following, contourArea by the shoelace sum, boundingRect and a filled rectangle whose
 * far corner is inclusive. Everything else is THIS PROJECT'S DEFINITION, rules C1-C6 below; the yardstick is
 * dsdtm_amd/contour_restatement.py and its plain-C twin tests/contour_restatement.c, bit-equal to each other, to mcd_box_host and to
 * the device on every test case (the step is integer-only). Parity with OpenCV is unpinned and stays unpinned; in particular
 * OpenCV's contour ORDER, which decides between contours of equal area, is unpinned.
 *
 *   C1 foreground   A pixel is foreground when its byte is non-zero (:104 on a 255 / 0 image). Components are 8-connected. Outside the
 *                   image is background.
 *   C2 contour      A component's contour is its OUTER border: the closed walk over 8-adjacent border pixels that
 *                   findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) lists. It is a Moore-neighbour trace that starts at the component's
 *                   raster-first pixel (lowest y, then lowest x), entered from its left neighbour: the neighbours are searched
 *                   clockwise from there for the walk's LAST pixel, then from each pixel counter-clockwise behind the pixel it was
 *                   entered from. It ends by Suzuki's rule: back at the start pixel and about to repeat the first move. A single pixel
 *                   is a contour of one point; thin parts are walked twice. Components nested in a hole of another may be traced or
 *                   skipped (the restatement traces them, the device skips what cannot win): their area is strictly smaller than the
 *                   enclosing contour's, so they never decide anything. n_components counts EVERY 8-connected component, nested ones
 *                   included (OpenCV's contours.size() does not count those).
 *   C3 area         area2 = | sum of (x_prev * y_cur - y_prev * x_cur) | over the closed walk, in int64: contourArea's double, doubled;
 *                   exact in integers.
 *   C4 winner       The component with the largest area2, and area2 must be > 0 (`area > maxArea` from 0, :112): a mask of dots and
 *                   lines draws nothing. Ties go to the component whose raster-first pixel has the lowest index.
 *   C5 rectangle    The winner's bounding box minx..maxx x miny..maxy INCLUSIVE (boundingRect :120; cv::rectangle fills up to
 *                   br - (1, 1) inclusive, :123), filled with 255 into a copy of the mask; every other byte is unchanged.
 *                   box = x, y, w, h = minx, miny, maxx - minx + 1, maxy - miny + 1; all zero when nothing is drawn.
 *   C6 features     feature_on_mask is the test of dsdtm_motion_step (cvRound, halves to even, == 255), made on the image WITH the
 *                   rectangle (src/Frame.cpp:352).
 */
#ifndef DSDTM_AMD_MCD_H
#define DSDTM_AMD_MCD_H

#include "dsdtm_amd_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_MCD_MAX_PIXELS 1048576        /* width * height of a mask that takes the contour step (its bit-plane lives in one workgroup's LDS) */

typedef struct dsdtm_mcd_ctx dsdtm_mcd_ctx;
int dsdtm_mcd_create(int device, dsdtm_mcd_ctx** out);
/* Models of the context must be destroyed first. */
void dsdtm_mcd_destroy(dsdtm_mcd_ctx* ctx);
const char* dsdtm_mcd_last_error(const dsdtm_mcd_ctx* ctx);

/* ---- the model: dsdtm_motion_model under this library's names, with the limits DSDTM_MOTION_* (sides 16 .. 4096). A model larger than
 * DSDTM_MCD_MAX_PIXELS can be made, read and written; the step entries below refuse it. ---- */
typedef struct dsdtm_mcd_model dsdtm_mcd_model;
int dsdtm_mcd_model_create(dsdtm_mcd_ctx* ctx, int width, int height, dsdtm_mcd_model** out);
void dsdtm_mcd_model_destroy(dsdtm_mcd_ctx* ctx, dsdtm_mcd_model* model);
int dsdtm_mcd_model_reset(dsdtm_mcd_ctx* ctx, dsdtm_mcd_model* model);
int dsdtm_mcd_model_read(dsdtm_mcd_ctx* ctx, const dsdtm_mcd_model* model, float* out);
int dsdtm_mcd_model_write(dsdtm_mcd_ctx* ctx, dsdtm_mcd_model* model, const float* in);

/* ---- the whole MCDWrapper::Run for n independent models in ONE submission ----------------------------------------------------
 * One upload, the step kernel, the contour kernels, the fill, the feature lookup on the image WITH the rectangle, the read-back, one
 * wait. The fields a dsdtm_motion_desc has mean what they mean there, except:
 *   mask         host memory, rows mask_stride >= width apart, NULL = not wanted: the image WITH the rectangle (what Run returns)
 *   mask_raw     host memory, rows mask_raw_stride >= width apart, NULL = not wanted: detect_img BEFORE the rectangle, exactly what
 *                dsdtm_motion_step returns
 *   box, area2, n_components   OUTPUTS, written into the desc: C5's x, y, w, h (all zero when no rectangle is drawn), C3's value of the
 *                winner (0 when there is none), the number of 8-connected components of detect_img
 * 0 <= n <= DSDTM_MOTION_STEPS_MAX (n == 0: DSDTM_OK, nothing done); the same model twice is an error; a model of more than
 * DSDTM_MCD_MAX_PIXELS pixels returns DSDTM_ERR_INVALID naming the size. All or nothing: everything is checked before anything is
 * enqueued; after any failure no output (the descs' fields included) is touched and no model has turned over. Each result is
 * bit-equal to its single dsdtm_mcd_step. */
typedef struct dsdtm_mcd_desc {
    dsdtm_mcd_model* model;
    const uint8_t* image; int32_t stride;
    int32_t mask_stride; uint8_t* mask;
    const double* H;
    int32_t n_features; int32_t mask_raw_stride;
    const float* feature_px; uint8_t* feature_on_mask;
    uint8_t* mask_raw;
    int32_t box[4];
    int64_t area2;
    int32_t n_components; int32_t reserved;
} dsdtm_mcd_desc;
int dsdtm_mcd_steps(dsdtm_mcd_ctx* ctx, int n, dsdtm_mcd_desc* descs);
/* The same for one model. box: 4 int32; box, area2 and n_components may each be NULL. */
int dsdtm_mcd_step(dsdtm_mcd_ctx* ctx, dsdtm_mcd_model* model, const uint8_t* image, int stride, const double* H,
                   uint8_t* mask_raw, int mask_raw_stride, uint8_t* mask, int mask_stride,
                   int n_features, const float* feature_px, uint8_t* feature_on_mask, int32_t* box, int64_t* area2, int32_t* n_components);

/* ---- rules C1-C5 on n arbitrary 8-bit masks in ONE submission ------------------------------------------------------------------
 *   mask         width x height bytes, rows `stride` >= width apart, in host memory (copied into the upload) or in this device's
 *                memory (read where it is, never written). DSDTM_MOTION_MIN_SIDE <= width, height <= DSDTM_MOTION_MAX_SIDE and
 *                width * height <= DSDTM_MCD_MAX_PIXELS, else DSDTM_ERR_INVALID naming the size.
 *   boxed        host memory, rows boxed_stride >= width apart, NULL = not wanted: the mask with the rectangle
 *   box, area2, n_components   OUTPUTS, as above
 * 0 <= n <= DSDTM_MOTION_STEPS_MAX. All or nothing. */
typedef struct dsdtm_mcd_box_desc {
    const uint8_t* mask; int32_t width, height; int32_t stride;
    int32_t boxed_stride; uint8_t* boxed;
    int32_t box[4];
    int64_t area2;
    int32_t n_components; int32_t reserved;
} dsdtm_mcd_box_desc;
int dsdtm_mcd_boxes(dsdtm_mcd_ctx* ctx, int n, dsdtm_mcd_box_desc* descs);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_MCD_H */
