/*
 * dsdtm_amd_undistort.h — C ABI of libdsdtm_amd_undistort.so: rectification of raw RGB-D frames (gray and depth) and of feature pixels
 * on the MI355X (gfx950), the step between a raw sensor frame and dsdtm_frame_prefetch.
 *
 * An ADD-ON library beside libdsdtm_amd.so, like the other dsdtm_amd_*.h: a header, a context and sources of its own, so that the
 * surfaces of those libraries stay exactly what they are. It shares their conventions — POD arguments, caller-owned memory, `int`
 * status returns (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling thread, NO CPU fallback — and
 * nothing else: a dsdtm_undistort_ctx owns its own stream and staging block.
 *
 * Replaces: cv::undistort(tColorImg, mColorImg, K, D, K), which the reference switched off for its cost alone (src/Frame.cpp:57-61,
 *           "it takes almost 6ms to undistort the image"), and Frame::UndistortFeatures (src/Frame.cpp:94-150), which it runs instead
 *           from CreateInitialMapRGBD (src/Tracking.cpp:149) and CraeteKeyframe (:417): cv::undistortPoints(.., K, D, noArray(), K) on
 *           every non-initial feature and its bearing recomputed. K is Camera::mInstrinsicMat, D is Camera::mDistortionMat
 *           (k1 k2 p1 p2 k3, src/Camera.cpp:62-67); Config/kinect.yaml carries a distortion that is not zero.
 *           Every other entry of this project is defined for RECTIFIED images (include/dsdtm_amd_newkf.h says so in two places:
 *           "cv::undistortPoints ... is NOT restated" and "defined for RECTIFIED images"); those sentences stay true of that library.
 *           A frame that went through dsdtm_undistort_frames IS rectified, and its device destination is handed to
 *           dsdtm_frame_prefetch / dsdtm_track_frame as it is (include/dsdtm_amd.h, "The caller's buffers").
 *
 * PARITY. OpenCV is not available to this project, in source or binary. What is kept is the documented shape of the OpenCV calls
 * (initUndistortRectifyMap with R = I and P = K, remap with INTER_LINEAR at INTER_BITS = 5 and BORDER_CONSTANT 0, undistortPoints with
 * five fixed iterations). Everything finer is THIS PROJECT'S DEFINITION, the numbered rules below; the yardstick is their numpy
 * restatement dsdtm_amd/undistort_restatement.py, to which the device and the host functions of dsdtm_amd/host/dsdtm_undistort_host.hpp
 * are bit-equal. Parity with OpenCV's fixed-point remap (its interpolation tables, its rounding of the weights) is unpinned and stays
 * unpinned.
 *
 * THE DEFINITION
 *   U1 the map   cv::undistort(src, dst, K, D, K) = initUndistortRectifyMap(K, D, I, K). fx fy cx cy are the float members of dsdtm_camera
 *                widened to double (mInstrinsicMat is CV_32F), the coefficients floats widened to double. For the destination pixel
 *                (u, v), in IEEE double, every multiply and add rounded on its own (never contracted), in this order:
 *                  1. x = (u - cx) / fx, y = (v - cy) / fy
 *                  2. r2 = x*x + y*y
 *                  3. radial = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *                  4. xd = x*radial + (((2*p1)*x)*y + p2*(r2 + (2*x)*x))
 *                  5. yd = y*radial + (p1*(r2 + (2*y)*y) + ((2*p2)*x)*y)
 *                  6. mx = xd*fx + cx, my = yd*fy + cy
 *                The stored map is fixed point at 1/32 pixel (INTER_BITS = 5): X = cvRound(mx * 32), Y = cvRound(my * 32), cvRound
 *                rounding halves to even, saturated to int32; a value that is not finite becomes DSDTM_UNDISTORT_OUTSIDE, which
 *                reads as "outside the source" in U2 and U3 (as both saturated ends do).
 *   U2 gray      integer bilinear, borders read 0. x0 = X >> 5, ax = X & 31, y0 = Y >> 5, ay = Y & 31 (arithmetic shifts); the taps
 *                p00 = src(y0, x0), p01 = src(y0, x0+1), p10 = src(y0+1, x0), p11 = src(y0+1, x0+1), a tap outside the source being 0;
 *                dst = ((32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11 + 512) >> 10. Nothing floats.
 *   U3 depth     u16, NEAREST neighbour on the same map: source pixel (floor((X + 16) / 32), floor((Y + 16) / 32)), evaluated as
 *                (X >> 5) + (((X & 31) + 16) >> 5) so that no X overflows; outside the source: 0, "no depth". No interpolation: mixing
 *                depth across an edge or with a 0 would invent surfaces. THIS IS THE PROJECT'S DEFINITION: the reference never remaps
 *                its depth image (it reads the raw depth at the undistorted pixel).
 *   U4 frames    dsdtm_undistort_frames below.
 *   U5 points    cv::undistortPoints(in, out, K, D, noArray(), K), in double, never contracted:
 *                  1. x0 = (u - cx)/fx, y0 = (v - cy)/fy (u, v: the float pixel widened); x = x0, y = y0
 *                  2. exactly FIVE times (the fixed count of the OpenCV 2.4 the reference builds against):
 *                       r2 = x*x + y*y; icdist = 1 / (1 + ((k3*r2 + k2)*r2 + k1)*r2);
 *                       dx = ((2*p1)*x)*y + p2*(r2 + (2*x)*x); dy = p1*(r2 + (2*y)*y) + ((2*p2)*x)*y;
 *                       x = (x0 - dx)*icdist; y = (y0 - dy)*icdist
 *                  3. x*fx + cx and y*fy + cy, each narrowed ONCE to float (the reference stores them in a CV_32F matrix).
 *                skip[i] != 0 is an mbInitial feature (src/Frame.cpp:141-142): its pixel is copied and its bearing NOT WRITTEN.
 *                Otherwise the bearing is Pixel2Camera(px, 1.0) normalised from the undistorted float pixel, in the float / double
 *                mix a new feature's bearing has everywhere in this project (include/dsdtm_amd_newkf.h K5):
 *                bx = (double)((1.0f*(px - cx))/fx), by likewise in float; nrm = sqrt(bx*bx + by*by + 1.0*1.0) in double; b = (bx, by, 1)/nrm.
 */
#ifndef DSDTM_AMD_UNDISTORT_H
#define DSDTM_AMD_UNDISTORT_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_UNDISTORT_MIN_SIDE 8
#define DSDTM_UNDISTORT_MAX_SIDE 4096
#define DSDTM_UNDISTORT_MAX_FRAMES 1024
#define DSDTM_UNDISTORT_MAX_POINTS 16384
#define DSDTM_UNDISTORT_OUTSIDE (-2147483647 - 1) /* a map entry that is not finite */

typedef struct dsdtm_undistort_ctx dsdtm_undistort_ctx;
typedef struct dsdtm_undistort_map dsdtm_undistort_map;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_undistort_create(int device, dsdtm_undistort_ctx** out);
void dsdtm_undistort_destroy(dsdtm_undistort_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_undistort_create when ctx == NULL). */
const char* dsdtm_undistort_last_error(const dsdtm_undistort_ctx* ctx);

/* U1: the map of cam->width x cam->height, built ONCE by a kernel on the context's device and kept there (8 bytes per pixel). dist:
 * k1 k2 p1 p2 k3. Refused (DSDTM_ERR_INVALID naming the field): a width or height below DSDTM_UNDISTORT_MIN_SIDE or above
 * DSDTM_UNDISTORT_MAX_SIDE, an intrinsic or a coefficient that is not finite, fx or fy not greater than 0. Synchronous. A map is used
 * with any context of the same device, by one thread at a time, and is destroyed before the last context of its device. */
int dsdtm_undistort_map_create(dsdtm_undistort_ctx* ctx, const dsdtm_camera* cam, const float dist[5], dsdtm_undistort_map** out);
void dsdtm_undistort_map_destroy(dsdtm_undistort_map* map);
/* The map as U1 defines it: width * height pairs (X, Y) of int32, row-major, into host memory. For tests. */
int dsdtm_undistort_map_read(dsdtm_undistort_ctx* ctx, const dsdtm_undistort_map* map, int32_t* xy_out);

/* One frame. gray_src / gray_dst: rows of the map's width bytes, `*_stride` bytes apart. depth_src / depth_dst: u16, strides in
 * ELEMENTS; both NULL: the frame has no depth (one of them NULL: refused). A source lies in pageable host memory (copied into the
 * context's pinned block and uploaded), in pinned host memory or in this device's memory (both read where they are). A destination lies
 * in this device's memory (written in place: ready for dsdtm_frame_prefetch when the call returns) or in host memory (read back).
 * hipPointerGetAttributes decides; another device's memory is refused.
 * STAGING MEMORY: every pageable source and every host destination of a call is packed (width * height elements) into the context's pinned
 * block AND into a device block of the same size; both grow to the request plus a quarter and are kept until the context is destroyed.
 * 1024 pageable 640 x 480 gray + depth frames are about 0.9 GB of each (1.9 GB with host destinations). Device and pinned sources and
 * device destinations are used in place and cost nothing here: large batches belong there. A block that cannot be had is DSDTM_ERR_HIP. */
typedef struct dsdtm_undistort_desc {
    const dsdtm_undistort_map* map;
    const uint8_t* gray_src;
    uint8_t* gray_dst;
    const uint16_t* depth_src;
    uint16_t* depth_dst;
    int32_t gray_src_stride, gray_dst_stride;   /* bytes    */
    int32_t depth_src_stride, depth_dst_stride; /* elements */
} dsdtm_undistort_desc;

/* U4: n frames (0 <= n <= DSDTM_UNDISTORT_MAX_FRAMES; n == 0: DSDTM_OK, nothing done) in ONE submission: one upload, ONE launch for all
 * frames, gray and depth together (the frame is a grid dimension; frames may differ in map and size), one read-back (where a destination
 * is host memory), one wait. SYNCHRONOUS ON PURPOSE: dsdtm_frame_prefetch runs on a stream of libdsdtm_amd.so that nothing outside it
 * can order against, so a device destination is complete when this call returns. Each frame of a batch is byte-equal to its single
 * call. Everything is checked before anything is enqueued and an error names the desc and the field; all or nothing (a host destination
 * is written after the wait only; after a DSDTM_ERR_HIP behind the launch the content of a DEVICE destination is undefined). Refused besides
 * the above: a stride below the width; a destination whose extent ((height - 1) * stride + width elements) overlaps the extent of any
 * source of the call or of any other destination of the call; a map of another device. Inside a stream capture: DSDTM_ERR_INVALID. */
int dsdtm_undistort_frames(dsdtm_undistort_ctx* ctx, int n, const dsdtm_undistort_desc* descs);

/* U5: n pixels (0 <= n <= DSDTM_UNDISTORT_MAX_POINTS; n == 0: DSDTM_OK, nothing done), all arrays in host memory. px_in, px_out:
 * n x 2 floats (px_out may be px_in); skip: n bytes or NULL (nothing skipped); bearing_out: n x 3 doubles, rows of skipped pixels
 * untouched. cam->width / height are not read. Refused: what dsdtm_undistort_map_create refuses of cam and dist; an input pixel that is
 * not finite (named by its index). Synchronous; all or nothing. For ONE tracker the host function undistort_points_host of
 * dsdtm_amd/host/dsdtm_undistort_host.hpp, bit-equal, is the faster way (profiles/r22_undistort.txt). */
int dsdtm_undistort_points(dsdtm_undistort_ctx* ctx, const dsdtm_camera* cam, const float dist[5], int n, const float* px_in,
                           const uint8_t* skip, float* px_out, double* bearing_out);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_UNDISTORT_H */
