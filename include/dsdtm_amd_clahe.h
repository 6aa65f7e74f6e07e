/*
 * dsdtm_amd_clahe.h — C ABI of libdsdtm_amd_clahe.so: contrast-limited adaptive histogram equalisation of 8-bit gray frames on the
 * MI355X (gfx950), the first thing the reference's drivers do to a frame and the step in front of dsdtm_frame_prefetch.
 *
 * An ADD-ON library beside libdsdtm_amd.so, like the other dsdtm_amd_*.h: a header, a context and sources of its own, so that the
 * surfaces of those libraries stay exactly what they are. It shares their conventions — POD arguments, caller-owned memory, `int`
 * status returns (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling thread, NO CPU fallback — and
 * nothing else: a dsdtm_clahe_ctx owns its own stream and staging block.
 *
 * Replaces: cv::createCLAHE(3.0, cv::Size(8, 8))->apply(Image, Image_tmp), which Test/test_Feature_detection.cpp:85-86,
 *           Test/test_Euroc.cpp:64-65 and Test/test_Optimizer.cpp:75-76 run on every image before Feature_detector::detect, and which
 *           Test/test_Tracking.cpp:78-79 and Test/test_uzhsin.cpp:122-123 carry commented out beside the note "The single image cost
 *           almost 10ms on reading and clahe" (:71, :114). A device destination of this library is handed to dsdtm_frame_prefetch,
 *           dsdtm_detect_cells_frame and dsdtm_undistort_frames as it is (include/dsdtm_amd.h, "The caller's buffers").
 *
 * PARITY. OpenCV is not available to this project, in source or binary. What is kept is the documented shape of cv::CLAHE::apply for
 * CV_8UC1 as of the OpenCV 2.4 the reference builds against (README.md:4): a grid of tiles over the image extended to a multiple of
 * the grid, a clipped and redistributed histogram per tile, a look-up table per tile, bilinear interpolation between the four nearest
 * tables. Everything finer is THIS PROJECT'S DEFINITION, the numbered rules below; the yardstick is their numpy restatement
 * dsdtm_amd/clahe_restatement.py, to which the device and the host functions of dsdtm_amd/host/dsdtm_clahe_host.hpp are bit-equal.
 * Parity with OpenCV binaries is unpinned and stays unpinned.
 *
 * THE DEFINITION
 *   E1 grid      tiles_x, tiles_y (0: 8), clip_limit (a double, taken literally). If width % tiles_x == 0 && height % tiles_y == 0 the
 *                histogram source is the image. Otherwise it is the image extended by tiles_x - width % tiles_x columns on the right
 *                AND tiles_y - height % tiles_y rows at the bottom with BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba, the mirror
 *                repeated where the extension is longer than the side less one). QUIRK kept: a side that does divide still gets a
 *                whole `tiles` of padding when the other side does not (64 x 50 at 8 x 8 is extended to 72 x 56). The tile is
 *                (ext_w / tiles_x) x (ext_h / tiles_y) pixels, `area` their product. The extension is never materialised by the
 *                device or the host function: both index by reflection (the restatement pads, so that it is independent of that).
 *   E2 clip      clip_limit > 0: clip = max((int)(clip_limit * area / 256), 1), product and quotient in double, truncated; a quotient
 *                at or above `area` is taken as `area` (no count is larger: nothing is clipped). clip_limit <= 0: no clipping.
 *   E3 histogram per tile, 256 int32 counts over the tile's `area` pixels of the (virtually) extended image.
 *   E4 clip and redistribute   clipped = sum of max(h[i] - clip, 0); h[i] = min(h[i], clip); batch = clipped / 256,
 *                residual = clipped - 256 * batch; every bin += batch; bins 0 .. residual-1 += 1. This is the rule of OpenCV 2.4. The
 *                STRIDED RESIDUAL of OpenCV 3.x (one count to every (256 / residual)-th bin) is NOT this definition.
 *   E5 table     scale = 255.0f / (float)area (one float division); lut[i] = saturate_u8(cvRound((float)cumsum_i * scale)), the
 *                cumulative sum in int32 and converted to float once, the multiply in float, cvRound rounding halves to even. With a
 *                side of at most DSDTM_CLAHE_MAX_SIDE and a single tile the sum stays at or below 2^24, so the conversion is exact.
 *   E6 interpolation   for the ORIGINAL width x height pixels only, in float, every operation rounded on its own (never contracted):
 *                inv_tw = 1.0f / tile_w; txf = x * inv_tw - 0.5f; tx1 = floor(txf); tx2 = tx1 + 1; xa = txf - tx1; then
 *                tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1); likewise for y. With v = src(y, x):
 *                res = lut[ty1][tx1][v] * ((1 - xa) * (1 - ya)) + lut[ty1][tx2][v] * (xa * (1 - ya)) + lut[ty2][tx1][v] * ((1 - xa) * ya)
 *                      + lut[ty2][tx2][v] * (xa * ya), summed left to right; dst = saturate_u8(cvRound(res)).
 *                (The nested form lerp(lerp, lerp) is NOT this definition: it rounds differently.)
 *   E7 frames    dsdtm_clahe_apply_batch below.
 */
#ifndef DSDTM_AMD_CLAHE_H
#define DSDTM_AMD_CLAHE_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_CLAHE_MIN_SIDE 16
#define DSDTM_CLAHE_MAX_SIDE 4096
#define DSDTM_CLAHE_MAX_TILES 16 /* per side */
#define DSDTM_CLAHE_DEFAULT_TILES 8
#define DSDTM_CLAHE_DEFAULT_CLIP_LIMIT 3.0
#define DSDTM_CLAHE_MAX_FRAMES 1024

typedef struct dsdtm_clahe_ctx dsdtm_clahe_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_clahe_create(int device, dsdtm_clahe_ctx** out);
void dsdtm_clahe_destroy(dsdtm_clahe_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_clahe_create when ctx == NULL). */
const char* dsdtm_clahe_last_error(const dsdtm_clahe_ctx* ctx);

/* One frame. src / dst: rows of `width` bytes, `*_stride` bytes apart. A source lies in pageable host memory (copied into the context's
 * pinned block and uploaded), in pinned host memory or in this device's memory (both read where they are). A destination lies in this
 * device's memory (written in place: ready for dsdtm_frame_prefetch when the call returns) or in host memory (read back).
 * hipPointerGetAttributes decides; another device's memory is refused. lut_out: NULL, or HOST memory of tiles_y * tiles_x * 256 bytes
 * that receives the tables of E5, table (ty, tx) at ((ty * tiles_x) + tx) * 256: for callers who reuse tables, and for tests.
 * clip_limit is taken literally (0: no clipping; the C++ and Python wrappers default it to DSDTM_CLAHE_DEFAULT_CLIP_LIMIT); tiles_x /
 * tiles_y: 0 means DSDTM_CLAHE_DEFAULT_TILES.
 * STAGING MEMORY: every pageable source, every host destination (packed, width * height bytes) and every requested lut_out of a call
 * lies in the context's pinned block AND in a device block, which holds every frame's tables besides (at most 64 KiB per frame); both
 * grow to the request plus a quarter and are kept until the context is destroyed. 1024 pageable 640 x 480 frames are about 0.3 GB of
 * each (0.6 GB with host destinations). Device and pinned sources and device destinations are used in place and cost nothing here:
 * large batches belong there. A block that cannot be had is DSDTM_ERR_HIP. */
typedef struct dsdtm_clahe_desc {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* lut_out;
    double clip_limit;
    int32_t width, height;
    int32_t src_stride, dst_stride; /* bytes */
    int32_t tiles_x, tiles_y;
} dsdtm_clahe_desc;

/* E7: n frames (0 <= n <= DSDTM_CLAHE_MAX_FRAMES; n == 0: DSDTM_OK, nothing done) of mixed sizes and parameters in ONE submission: one
 * upload, TWO launches for all frames (the tables, then the interpolation; the frame is a grid dimension), one read-back (where a
 * destination is host memory or tables are asked for), one wait. SYNCHRONOUS ON PURPOSE: dsdtm_frame_prefetch runs on a stream of
 * libdsdtm_amd.so that nothing outside it can order against, so a device destination is complete when this call returns. Each frame
 * of a batch is byte-equal to its single call. Everything is checked before anything is enqueued and an error names the desc and the
 * field; all or nothing (host memory is written after the wait only; after a DSDTM_ERR_HIP behind the launch the content of a DEVICE
 * destination is undefined). Refused with DSDTM_ERR_INVALID: a width or height below DSDTM_CLAHE_MIN_SIDE or above
 * DSDTM_CLAHE_MAX_SIDE; tiles_x or tiles_y outside 0..DSDTM_CLAHE_MAX_TILES; a clip_limit that is not finite or is negative; a stride
 * below the width; src or dst NULL; a destination (dst, lut_out) whose extent ((height - 1) * stride + width bytes) overlaps the extent
 * of any source of the call or of any other destination of the call; another device's memory; lut_out in device memory. Inside a
 * stream capture: DSDTM_ERR_INVALID. */
int dsdtm_clahe_apply_batch(dsdtm_clahe_ctx* ctx, int n, const dsdtm_clahe_desc* descs);
/* dsdtm_clahe_apply_batch(ctx, 1, desc). */
int dsdtm_clahe_apply(dsdtm_clahe_ctx* ctx, const dsdtm_clahe_desc* desc);
/* E1-E5 alone: the tables of one frame into desc->lut_out (required). There is no destination: dst and dst_stride are not read. One
 * launch; otherwise as dsdtm_clahe_apply. */
int dsdtm_clahe_luts(dsdtm_clahe_ctx* ctx, const dsdtm_clahe_desc* desc);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_CLAHE_H */
