/*
 * dsdtm_amd_framediff.h — C ABI of libdsdtm_amd_framediff.so: Moving_Detecter::Mod_FrameDiff — warp the other frame by H, subtract,
 * threshold, open and dilate — and the feature test of Frame::Motion_Removal on its mask, on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, like the other dsdtm_amd_*.h: a header, a context and sources of its own, so that the
 * surfaces of those libraries stay exactly what they are. It shares their conventions — POD arguments, caller-owned memory, `int`
 * status returns (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling thread, NO CPU fallback — and
 * nothing else: a dsdtm_framediff_ctx owns its own stream and staging block.
 *
 * Replaces: Moving_Detecter::Mod_FrameDiff (src/Moving_Detection.cpp:36-63) behind its findHomography (:47, which is
 *           dsdtm_find_homography's, include/dsdtm_amd_homography.h, or dsdtm_klt_step's, include/dsdtm_amd_klt.h):
 *           warpPerspective(tImgB, mMask, H, size) (:48), mMask = tImgA - mMask (:50, saturating u8), threshold(.., 50, 200.0,
 *           CV_THRESH_BINARY) (:52), morphologyEx(MORPH_OPEN, 5x5 rect) (:54-55), dilate(5x5 rect) (:56); and the test Frame::Motion_Removal
 *           makes per feature (src/Frame.cpp:352). Tracking::MotionRemoval chooses between this detector and Mod_FastMCD
 *           (src/Tracking.cpp:507-508). It is the stateless one: no model, usable from the second frame.
 * SUPERSEDES the sentences "out of scope: Moving_Detecter::Mod_FrameDiff" of include/dsdtm_amd_motion.h, include/dsdtm_amd_mcd.h and
 *           include/dsdtm_amd_homography.h, which stay true of THOSE libraries: with this one every part of Moving_Detecter has a
 *           counterpart on the device.
 *
 * TWO QUIRKS OF THE SOURCE, both kept and both the caller's to decide:
 *   QUIRK 1  :45 reads `tImgB = tframeA->mColorImg`: both images are frame A, so the reference warps frame A and subtracts it from
 *            itself. The entry takes two images a and b; a caller who wants the line to the letter passes b = a (the same pointer is
 *            allowed). The adapters (dsdtm_amd/mcd.py, dsdtm_amd/host/dsdtm_mcd_host.hpp) pass frame B and say so.
 *   QUIRK 2  the mask's foreground is 200 (:52) and Frame::Motion_Removal tests `!= 255` (src/Frame.cpp:352): with the reference's own
 *            constants NO feature is ever removed by a FrameDiff mask. Kept: `maxval` is an argument, 0 means
 *            DSDTM_FRAMEDIFF_MAXVAL = 200, and feature_on_mask is the `== 255` test of dsdtm_motion_step — at 200 it is all zero. A
 *            caller who wants the mask to act passes 255.
 *
 * PARITY. OpenCV is not available to this project, in source or binary. What is kept is the documented shape of the calls: INTER_LINEAR
 * at INTER_BITS = 5, BORDER_CONSTANT 0, H inverted unless WARP_INVERSE_MAP, THRESH_BINARY strictly greater, morphology whose default
 * border takes no part in the min / max. Everything finer is THIS PROJECT'S DEFINITION, rules F1-F8 below; the yardstick is their numpy
 * restatement dsdtm_amd/framediff_restatement.py, to which the device and frame_diff_host / warp_perspective_host of
 * dsdtm_amd/host/dsdtm_framediff_host.hpp are bit-equal in every byte, M included. Parity with warpPerspective's fixed-point tables is
 * unpinned and stays unpinned.
 *
 * THE DEFINITION
 *   F1 matrix      With DSDTM_FRAMEDIFF_INVERSE_MAP set M = H (H maps a destination pixel to the source: dsdtm_klt_step's direction when
 *                  a is the current image and b the previous one). Otherwise M = inverse of H, on the host in IEEE double, every
 *                  product and sum rounded on its own and never contracted, in this order:
 *                    det = h0*(h4*h8 - h5*h7) - h1*(h3*h8 - h5*h6) + h2*(h3*h7 - h4*h6), left to right; d = 1/det;
 *                    M0 = (h4*h8-h5*h7)*d  M1 = (h2*h7-h1*h8)*d  M2 = (h1*h5-h2*h4)*d
 *                    M3 = (h5*h6-h3*h8)*d  M4 = (h0*h8-h2*h6)*d  M5 = (h2*h3-h0*h5)*d
 *                    M6 = (h3*h7-h4*h6)*d  M7 = (h1*h6-h0*h7)*d  M8 = (h0*h4-h1*h3)*d
 *                  det == 0, or any h or M not finite: DSDTM_ERR_INVALID naming the desc index; nothing is enqueued. M is returned.
 *   F2 map         For the destination pixel (x, y), in double, not contracted: X0 = (M0*x + M1*y) + M2, Y0 = (M3*x + M4*y) + M5,
 *                  W = (M6*x + M7*y) + M8; s = W != 0 ? 32/W : 0; fX = X0*s, fY = Y0*s. A NaN becomes DSDTM_UNDISTORT_OUTSIDE's meaning
 *                  ("outside": -2^31); otherwise clamp to [-2^31, 2^31 - 1], then cvRound (halves to even): X, Y at 1/32 pixel.
 *                  Evaluated per pixel; no map is stored.
 *   F3 sample      warped(x, y) is rule U2 of include/dsdtm_amd_undistort.h on image b at (X, Y): x0 = X >> 5, ax = X & 31 (likewise y),
 *                  integer bilinear of the four taps, a tap outside b reading 0, + 512 >> 10.
 *   F4 difference  d = max(a(x, y) - warped(x, y), 0).
 *   F5 threshold   t = d > threshold, strict. threshold 0..254; the reference's is DSDTM_FRAMEDIFF_THRESHOLD = 50 and the entry uses the
 *                  field AS GIVEN (0 is the threshold 0, not a default).
 *   F6 morphology  The element is 5x5, its anchor in the centre; positions outside the image take no part in any of the three passes:
 *                  e(x, y) = AND of t over the window clipped to the image; o = OR of e over the clipped window; f = OR of o over the
 *                  clipped window. Consequences: a 3-pixel-wide strip along an image edge survives the erosion (at the edge column) and
 *                  comes out 5 wide; a 4x4 block anywhere vanishes; an interior 5x5 block comes out 9x9.
 *   F7 mask        byte = f ? maxval : 0. maxval 1..255; 0 means DSDTM_FRAMEDIFF_MAXVAL = 200.
 *   F8 features    feature_on_mask[i] = 1 when the mask at (cvRound(x), cvRound(y)) is 255: the rounding (halves to even, in float) and
 *                  the out-of-image rule (refused, naming the feature) of dsdtm_motion_step. n_foreground = the number of pixels with f
 *                  set; n_flagged = the sum of the flags.
 */
#ifndef DSDTM_AMD_FRAMEDIFF_H
#define DSDTM_AMD_FRAMEDIFF_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_FRAMEDIFF_MIN_SIDE 16
#define DSDTM_FRAMEDIFF_MAX_SIDE 4096
#define DSDTM_FRAMEDIFF_MAX_FEATURES 16384
#define DSDTM_FRAMEDIFF_MAX_STEPS 1024
#define DSDTM_FRAMEDIFF_THRESHOLD 50
#define DSDTM_FRAMEDIFF_MAXVAL 200
#define DSDTM_FRAMEDIFF_INVERSE_MAP 1 /* flags: H maps destination -> source (cv::WARP_INVERSE_MAP) */

typedef struct dsdtm_framediff_ctx dsdtm_framediff_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_framediff_create(int device, dsdtm_framediff_ctx** out);
void dsdtm_framediff_destroy(dsdtm_framediff_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_framediff_create when ctx == NULL). */
const char* dsdtm_framediff_last_error(const dsdtm_framediff_ctx* ctx);

/* One pair of gray images. a, b: width x height bytes, rows a_stride / b_stride bytes apart, each in pageable host memory (copied into
 * the context's pinned block and uploaded), pinned host memory or this device's memory (both read where they are);
 * hipPointerGetAttributes decides, another device's memory is refused. b == a is allowed (QUIRK 1) and is then staged once.
 *   mask       width x height bytes, rows mask_stride apart, in host memory (read back) or this device's memory (written in place);
 *              NULL: not wanted, and then it does not cross the link (the feature test reads a device copy). Bytes of a row beyond
 *              width are not touched.
 *   warped     optional, same rules: the image of F3.
 *   features   n_features x 2 floats (x, y) and n_features bytes, both in HOST memory, 0 <= n_features <= DSDTM_FRAMEDIFF_MAX_FEATURES.
 * Refused (DSDTM_ERR_INVALID naming the desc index and the field; everything is checked before anything is enqueued): a NULL a or b; a
 * side outside DSDTM_FRAMEDIFF_MIN_SIDE..MAX_SIDE; a stride below the width; flags with unknown bits; threshold outside 0..254; maxval
 * outside 0..255; what F1 refuses; a feature that is not finite or rounds outside the image; an output whose extent overlaps an input
 * or another output of the call. */
typedef struct dsdtm_framediff_desc {
    const uint8_t* a;
    const uint8_t* b;
    int32_t width, height, a_stride, b_stride;
    double H[9];
    int32_t flags, threshold, maxval, mask_stride;
    uint8_t* mask;
    uint8_t* warped;
    int32_t warped_stride, n_features;
    const float* feature_px;
    uint8_t* feature_on_mask;
} dsdtm_framediff_desc;

typedef struct dsdtm_framediff_result {
    double M[9];            /* F1: the matrix the map was evaluated with */
    int32_t n_foreground;   /* pixels with f set */
    int32_t n_flagged;      /* features on a 255 */
} dsdtm_framediff_result;

/* n independent pairs (0 <= n <= DSDTM_FRAMEDIFF_MAX_STEPS; n == 0: DSDTM_OK, nothing done), sizes may differ, in ONE submission: one
 * upload, ONE launch that carries F2-F7 for the whole batch (no intermediate image reaches global memory unless warped was asked for),
 * one of the feature test behind it, one read-back, one wait. Each result is bit-equal to its single call. All or nothing: after any
 * failure no output is written (after a DSDTM_ERR_HIP behind the launch the content of a DEVICE output is undefined). Inside a stream
 * capture: DSDTM_ERR_INVALID. */
int dsdtm_framediff_steps(dsdtm_framediff_ctx* ctx, int n, const dsdtm_framediff_desc* descs, dsdtm_framediff_result* results);
/* One pair. */
int dsdtm_framediff_step(dsdtm_framediff_ctx* ctx, const dsdtm_framediff_desc* desc, dsdtm_framediff_result* result);
/* The stateless cv::warpPerspective for gray images: F1-F3 alone, b -> warped (required here; host or device memory). a, threshold, maxval,
 * mask and the features are not read. One submission for the n descs. */
int dsdtm_framediff_warp(dsdtm_framediff_ctx* ctx, int n, const dsdtm_framediff_desc* descs);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_FRAMEDIFF_H */
