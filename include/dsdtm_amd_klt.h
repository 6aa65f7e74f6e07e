/*
 * dsdtm_amd_klt.h — C ABI of libdsdtm_amd_klt.so: KLTWrapper::RunTrack — the pyramidal Lucas-Kanade flow of a grid of points and the
 * homography of the points that survived — for n trackers in one submission on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, like the ten before it: a header, a context and sources of its own, so that the surfaces of
 * those libraries stay exactly what they are. It shares their conventions — POD arguments, caller-owned memory, `int` status returns
 * (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling thread, NO CPU fallback (the host evaluation
 * is dsdtm_amd/host/dsdtm_klt_host.hpp, which needs no library). It links homography.hip and pyrdown.hip as they are.
 *
 * Replaces: KLTWrapper::Init / InitFeatures / RunTrack / MakeHomoGraphy (Thirdparty/fastMCD/src/KLTWrapper.cpp:51-189), which MCDWrapper
 *           owns (MCDWrapper.h:59, MCDWrapper.cpp:75), and cv::calcOpticalFlowPyrLK as Test/test_Optimizer.cpp:91 calls it.
 *           include/dsdtm_amd_motion.h and include/dsdtm_amd_homography.h name KLTWrapper as out of scope; those sentences are pinned to
 *           their libraries and stay. THIS HEADER SUPERSEDES THEM: images -> H is dsdtm_klt_step, and its H is the argument that
 *           dsdtm_motion_step and dsdtm_mcd_step take (72 bytes, through the host).
 *
 * PARITY. OpenCV is not available to this project, in source or binary, so parity with cvCalcOpticalFlowPyrLK is
 * unpinned and stays unpinned. What is kept is the documented shape of the call at KLTWrapper.cpp:125-126: a 10 x 10 window, maxLevel 3 (4 levels made by
 * pyrDown), at most 20 iterations or a step of at most 0.03 px, Scharr derivatives, the minimum-eigenvalue test at 1e-4, the halved last
 * step on oscillation, status 0 for a point whose window leaves level 0. Everything else is THIS PROJECT'S DEFINITION, K1-K9 below.
 * The yardstick is dsdtm_amd/klt_restatement.py; klt_flow_host (dsdtm_klt_host.hpp) and the device are bit-equal to it.
 *
 * THE DEFINITION
 *   K1 pyramid   level 0 is the image; level l + 1 is pyrdown.hip's pyrDown of level l ([1 4 6 4 1] twice, BORDER_REFLECT_101,
 *                (sum + 128) >> 8, size ((w + 1) / 2, (h + 1) / 2)): the bytes dsdtm_pyrdown makes. A point p of level 0 is p / 2^l on
 *                level l (exact in double). (KLTWrapper.cpp:125: maxLevel 3.)
 *   K2 gradient  integer Scharr on the u8 level: gx(x, y) = 3 (I(x+1, y-1) - I(x-1, y-1)) + 10 (I(x+1, y) - I(x-1, y)) + 3 (I(x+1, y+1) -
 *                I(x-1, y+1)), gy likewise along y; |g| <= 4080. Not normalised.
 *   K3 sampling  the window of a point q on a level has its first tap at (ix, iy) = floor(q - (window - 1) / 2); with (fx, fy) the
 *                fraction, the four weights are integers in 1/2^14 (OpenCV's W_BITS): w00 = floor((1-fx)(1-fy) 2^14 + 0.5),
 *                w01 = floor(fx (1-fy) 2^14 + 0.5), w10 = floor((1-fx) fy 2^14 + 0.5), w11 = 2^14 - w00 - w01 - w10 (round half up; the
 *                products in double, left to right). A window value is (sum of 4 taps x weights + 2^8) >> 9 (5 fractional bits kept), a
 *                gradient value (sum + 2^13) >> 14; >> is the arithmetic shift (floor).
 *   K4 border    the window of the previous image, COUNTING THE 1-PIXEL SCHARR RING, must lie on the level: ix - 1 >= 0, iy - 1 >= 0,
 *                ix + window + 1 <= w - 1, iy + window + 1 <= h - 1 (the + 1: the bilinear tap). The window of the current image needs
 *                no ring: ix >= 0 ... ix + window <= w - 1. A window that leaves LEVEL 0 gives status 0. On a coarser level: a previous
 *                window that leaves it skips the level, a current window that leaves it ends the level's iterations; the guess is handed
 *                down as it stands either way. No pixel outside a level is read.
 *   K5 matrix    A11 = sum gx gx, A12 = sum gx gy, A22 = sum gy gy over the window: INTEGER sums in int64, so their order is free (the
 *                device reduces them across a wavefront). Bound for the largest window: 441 x 4080^2 < 2^33, and for the right-hand side
 *                441 x 8160 x 4080 < 2^34; a lane's own partial sum (7 terms) fits 32 bits. Each sum goes to double once and is multiplied
 *                by 2^-20 (exact). det = a11 a22 - a12 a12; min_eig = (a22 + a11 - sqrt((a11 - a22)(a11 - a22) + 4 a12 a12)) / (2 window^2).
 *                min_eig < 1e-4 or det < 2^-23: status 0 at level 0, the level skipped otherwise.
 *   K6 iteration from the level's guess q: b1 = sum (J - I) gx, b2 = sum (J - I) gy (int64, J the current window sampled at q by K3);
 *                dx = (a12 b2 - a22 b1) (1 / det), dy = (a12 b1 - a11 b2) (1 / det); q = q + d. Stop when dx dx + dy dy <= 0.03^2 (<=), or
 *                after 20 iterations, or — from the second iteration — when |dx + dx'| < 0.01 and |dy + dy'| < 0.01 against the step
 *                before (oscillation): then q = q - d 0.5. IEEE double, this order, no contraction.
 *   K7 levels    coarsest first. The first guess is the point itself (or the caller's guess) / 2^(levels - 1); a level hands q x 2 down.
 *                After level 0 the window at the final q is looked at once more: outside (K4), status 0; else residual = sum |J - I| /
 *                (32 window^2), the mean absolute difference in grey levels. Points and residual are rounded to float32 once, at the end;
 *                `iterations` counts the iterations of all levels.
 *   K8 grid      the points InitFeatures writes (KLTWrapper.cpp:102-107): (i gw + gw / 2, j gh + gh / 2) for i < W / gw - 1, j < H / gh - 1,
 *                i major; gw / gh of 0 mean 32 / 24. QUIRK NOT KEPT: the reference sets count = W / gw * H / gh (:99), more than it
 *                fills (400 against 361 at 640 x 480), so its tail is stale or uninitialised memory: there is nothing defined to restate.
 *   K9 H         the points with status 1, in ascending index, go to homography.hip's RANSAC (the definition of
 *                include/dsdtm_amd_homography.h) with A = current, B = previous — H maps the current frame to the last one, the direction
 *                dsdtm_motion_step expects ("REVERSE HOMOGRAPHY", KLTWrapper.cpp:162-189) — at a threshold of 1.0 px (:180) and that
 *                header's default confidence, hypothesis cap and seed. Fewer than 10 tracked points: the identity (:138-145). A RANSAC
 *                that finds nothing KEEPS THE MODEL'S PREVIOUS H: MakeHomoGraphy returns without writing matH (:180-184); this quirk is
 *                kept. `source` says which of the three happened. The first step of a model has no previous image: it returns the
 *                identity, tracks nothing (n_tracked = 0) and seeds the model.
 */
#ifndef DSDTM_AMD_KLT_H
#define DSDTM_AMD_KLT_H

#include "dsdtm_amd.h"
#include "dsdtm_amd_homography.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_KLT_MAX_STEPS 1024
#define DSDTM_KLT_MAX_FLOW_POINTS 16384
#define DSDTM_KLT_MAX_LEVELS 5
#define DSDTM_KLT_MIN_WINDOW 3
#define DSDTM_KLT_MAX_WINDOW 21
#define DSDTM_KLT_WINDOW 10            /* what dsdtm_klt_steps uses, and 0 in a flow desc means */
#define DSDTM_KLT_LEVELS 4
#define DSDTM_KLT_ITERATIONS 20
#define DSDTM_KLT_EPSILON 0.03
#define DSDTM_KLT_MIN_EIG 1e-4
#define DSDTM_KLT_MIN_TRACKED 10
#define DSDTM_KLT_RANSAC_THRESHOLD 1.0
#define DSDTM_KLT_SOURCE_IDENTITY 0
#define DSDTM_KLT_SOURCE_RANSAC 1
#define DSDTM_KLT_SOURCE_KEPT 2

typedef struct dsdtm_klt_ctx dsdtm_klt_ctx;
typedef struct dsdtm_klt_model dsdtm_klt_model;

/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_klt_create(int device, dsdtm_klt_ctx** out);
void dsdtm_klt_destroy(dsdtm_klt_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_klt_create when ctx == NULL). */
const char* dsdtm_klt_last_error(const dsdtm_klt_ctx* ctx);

/* A model: the device-resident pyramid of the previous image (the reference's CV_LKFLOW_PYR_A_READY), the previous H and a frame
 * counter. levels 1..DSDTM_KLT_MAX_LEVELS (0: DSDTM_KLT_LEVELS). DSDTM_ERR_INVALID, naming the field, where the coarsest level cannot
 * hold one 10 x 10 window and its ring (fewer than 13 pixels either way). reset: as created (the next step is a first step). */
int dsdtm_klt_model_create(dsdtm_klt_ctx* ctx, int width, int height, int levels, dsdtm_klt_model** out);
void dsdtm_klt_model_destroy(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model);
int dsdtm_klt_model_reset(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model);
/* Level `level` of the model's previous pyramid into host memory (width_l x height_l bytes, rows dst_stride apart): what the last step
 * built from its image. A DIAGNOSTIC entry (tests compare it with dsdtm_pyrdown's bytes): it waits for the context's stream.
 * DSDTM_ERR_INVALID before the first step. */
int dsdtm_klt_model_pyramid(dsdtm_klt_ctx* ctx, const dsdtm_klt_model* model, int level, uint8_t* dst, int dst_stride);

/* One RunTrack. image: width x height gray bytes, rows `stride` apart, in pageable, pinned or this device's memory. grid_w / grid_h: K8
 * (0: 32 / 24); the grid may hold DSDTM_HOMOGRAPHY_MAX_POINTS points at most. The four arrays are optional HOST arrays (NULL: not
 * wanted, and then the correspondences do not cross the link): prev_points / points n_points x 2 floats, status n_points bytes,
 * iterations n_points int32, mask n_points bytes of which the first n_tracked are written when source is RANSAC (the RANSAC model's
 * inlier flag per surviving point, in ascending point index). On a first step points = prev_points, status and iterations are 0. */
typedef struct dsdtm_klt_desc {
    dsdtm_klt_model* model;
    const uint8_t* image;
    int32_t stride;
    int32_t grid_w, grid_h;
    int32_t reserved;
    float* prev_points;
    float* points;
    uint8_t* status;
    int32_t* iterations;
    uint8_t* mask;
} dsdtm_klt_desc;

/* Every field is written by a call that returns DSDTM_OK. H: 9 doubles, row-major. With source != RANSAC the RANSAC fields are 0. */
typedef struct dsdtm_klt_result {
    double H[9];
    double cost_before, cost_after;
    int32_t source, n_points, n_tracked, n_inliers;
    int32_t best_hypothesis, rounds, refit_iterations, frame;      /* frame: the model's counter before this step (0: a first step) */
} dsdtm_klt_result;

/* n independent models (0 <= n <= DSDTM_KLT_MAX_STEPS) in ONE submission and one wait: images up, the pyramids (one pyrDown launch per
 * model and level), ONE Lucas-Kanade launch over all models' points, one compaction launch that writes the surviving correspondences
 * and their count into the homography records on the device, homography.hip's launch behind it, one read-back; then the pyramids are
 * swapped. Each result is bit-equal to its single call. A model may appear once per call: twice is refused. Everything is validated
 * before anything is enqueued, a failure names the index and the field; all or nothing: after any failure every output and every
 * model is as it was. Inside a stream capture: DSDTM_ERR_INVALID. */
int dsdtm_klt_steps(dsdtm_klt_ctx* ctx, int n, const dsdtm_klt_desc* descs, dsdtm_klt_result* results);
int dsdtm_klt_step(dsdtm_klt_ctx* ctx, dsdtm_klt_model* model, const uint8_t* image, int stride, dsdtm_klt_result* result);

/* The stateless primitive (cv::calcOpticalFlowPyrLK): n_points <= DSDTM_KLT_MAX_FLOW_POINTS points of the caller between two images of
 * one size (each in pageable, pinned or this device's memory). window 3..21, levels 1..5, iterations 1..100, epsilon, min_eig: 0 means
 * the DSDTM_KLT_* default. guesses: NULL, or where to start (OPTFLOW_USE_INITIAL_FLOW). Outputs, host arrays: out_points (required),
 * status, iterations_used, residual (optional). Refused, naming the field: a coarsest level too small for one window plus its ring. */
typedef struct dsdtm_klt_flow_desc {
    const uint8_t* prev;
    const uint8_t* cur;
    int32_t width, height, prev_stride, cur_stride;
    int32_t n_points, window, levels, iterations;
    double epsilon, min_eig;
    const float* points;
    const float* guesses;
    float* out_points;
    uint8_t* status;
    int32_t* iterations_used;
    float* residual;
} dsdtm_klt_flow_desc;

/* n pairs (0 <= n <= DSDTM_KLT_MAX_STEPS) in one submission and one wait; validated first, all or nothing, as above. */
int dsdtm_klt_flow(dsdtm_klt_ctx* ctx, int n, const dsdtm_klt_flow_desc* descs);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_KLT_H */
