/*
 * dsdtm_amd_homography.h — C ABI of libdsdtm_amd_homography.so: RANSAC homographies for n trackers in one launch on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, like libdsdtm_amd_keyframe.so and libdsdtm_amd_motion.so: a header, a context and sources of
 * its own, so that the surfaces of those libraries stay exactly what they are. It shares their conventions — POD arguments, caller-owned
 * memory, `int` status returns (the DSDTM_* codes), no exceptions, no globals, no environment, one context per calling thread, NO CPU
 * fallback — and nothing else: a dsdtm_homography_ctx owns its own stream and staging block.
 *
 * Replaces: cv::findHomography(tPointsA, tPointsB, CV_RANSAC) as Moving_Detecter::Mod_FastMCD calls it (src/Moving_Detection.cpp:28;
 *           Mod_FrameDiff makes the same call at :47, and KLTWrapper.cpp:180 calls the same function): the H that dsdtm_motion_step
 *           (include/dsdtm_amd_motion.h) takes as an argument. This is the missing half of Mod_FastMCD.
 *
 * PARITY. OpenCV is not available to this project, in source or binary. Therefore neither cv::findHomography's random sequence nor its
 * final refinement can be restated faithfully (the motion header says the same of findContours). What is kept is the documented shape
 * of findHomography(..., CV_RANSAC) at its default arguments: 4-point samples, forward reprojection error against 3 px, confidence 0.995,
 * about 2000 hypotheses at most, a refit on the inliers of the best model, the mask of the RANSAC model returned. Everything else is
 * THIS PROJECT'S DEFINITION: which samples are drawn, how ties fall, when the loop stops and how the refit iterates. The yardstick is
 * the float64 restatement dsdtm_amd/homography_restatement.py and its plain-C twin tests/homography_restatement.c: the two are bit-equal
 * to each other and the device is bit-equal to both, H included. Parity with OpenCV is unpinned and stays unpinned.
 *
 * THE DEFINITION (every decision rests on + - * / sqrt in IEEE double, without contraction, in one order of operations):
 *   problem     m correspondences A (current frame) -> B (last frame), float32 (x, y), widened once to double. H maps A to B: the
 *               direction dsdtm_motion_step expects ("maps a cell centre of the current frame to where its model lies").
 *               m <= 4: found = 0 and NOTHING ELSE is written for that problem (the reference's size() > 4).
 *               m <= DSDTM_HOMOGRAPHY_MAX_POINTS. A coordinate that is not finite: DSDTM_ERR_INVALID naming the problem and the index.
 *   sampling    counter-based: index = (hash(seed, hypothesis, draw) * m) >> 32 with the 32-bit integer hash
 *               x = seed + hypothesis * 0x9E3779B9 + draw * 0x85EBCA6B; x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16.
 *               A draw that repeats an index of the same sample is redrawn with the next counter; after 16 draws the hypothesis is
 *               invalid. Hypothesis k is the same whichever lane or round evaluates it.
 *   solver      closed form through the projective basis (for each image [p1 p2 p3] lambda = p4 by the adjugate, columns scaled,
 *               H = B_basis * adj(A_basis)), fixed order, no pivoting, normalised by H[8]. Invalid: a basis determinant or a lambda that
 *               is zero or not finite (three collinear points), H[8] zero, an entry not finite.
 *   score       a point is an inlier when |B - pi(H A)|^2 <= thr^2 (<=, not <). An invalid hypothesis scores -1. Best is the largest
 *               count; TIES GO TO THE LOWEST HYPOTHESIS INDEX.
 *   rounds      hypotheses come in rounds of 256, up to max_hypotheses rounded UP to whole rounds. After round r with best count c: stop
 *               when c == m or q^(256 r) <= 1.0 - confidence, w = c / m, q = 1 - (w w)(w w), the power by eight squarings and r - 1
 *               multiplications (no log, no pow). The rule is evaluated per ROUND, not per hypothesis. If no valid hypothesis has at
 *               least 4 inliers after the last round: found = 0, nothing else written — where OpenCV would return an EMPTY matrix, which
 *               the reference dereferences unchecked (H.ptr<double>(0), src/Moving_Detection.cpp:30).
 *   refit       Gauss-Newton on the forward reprojection error of the best model's inliers over the 8 free entries (H[8] = 1), both point
 *               sets Hartley-normalised for the solve, H de-normalised at the end; at most 10 iterations, each solving the 8x8 normal
 *               equations by Cholesky; a non-positive pivot, a non-finite step or a cost that does not fall ends the refit and keeps the
 *               last accepted H (with no accepted step: the RANSAC model, bit for bit). Sums over the inliers have a fixed shape (256
 *               strided partials in index order, then a tree), so a result does not depend on its place in a batch.
 *   outputs     THE MASK IS THE RANSAC MODEL'S, NOT RE-EVALUATED AFTER THE REFIT (1 / 0 per correspondence). cost_before / cost_after:
 *               the summed squared forward error of the inliers, in px^2, evaluated in the normalised frame and scaled back, before
 *               and after the refit (cost_after <= cost_before).
 */
#ifndef DSDTM_AMD_HOMOGRAPHY_H
#define DSDTM_AMD_HOMOGRAPHY_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_HOMOGRAPHY_MAX_POINTS 2048
#define DSDTM_HOMOGRAPHY_MAX_PROBLEMS 1024
#define DSDTM_HOMOGRAPHY_MAX_HYPOTHESES 4096
#define DSDTM_HOMOGRAPHY_DEFAULT_HYPOTHESES 2048
#define DSDTM_HOMOGRAPHY_DEFAULT_THRESHOLD 3.0
#define DSDTM_HOMOGRAPHY_DEFAULT_CONFIDENCE 0.995
#define DSDTM_HOMOGRAPHY_DEFAULT_SEED 0x2545F491u

typedef struct dsdtm_homography_ctx dsdtm_homography_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_homography_create(int device, dsdtm_homography_ctx** out);
void dsdtm_homography_destroy(dsdtm_homography_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_homography_create when ctx == NULL). */
const char* dsdtm_homography_last_error(const dsdtm_homography_ctx* ctx);

/* One problem. points_a / points_b: m x 2 floats (x, y) in host memory. mask: m bytes in host memory or NULL (not wanted).
 * reproj_threshold <= 0, confidence <= 0, max_hypotheses <= 0 and seed == 0 mean the defaults above; confidence must be below 1 and
 * max_hypotheses at most DSDTM_HOMOGRAPHY_MAX_HYPOTHESES. */
typedef struct dsdtm_homography_desc {
    const float* points_a;
    const float* points_b;
    uint8_t* mask;
    int32_t m;
    int32_t max_hypotheses;
    double reproj_threshold;
    double confidence;
    uint32_t seed;
    uint32_t reserved;
} dsdtm_homography_desc;

/* found = 0: no other field is written (and no byte of the mask). H: 9 doubles, row-major, H[8] = 1. best_hypothesis: the index of the
 * winning hypothesis; rounds: rounds of 256 hypotheses that ran; refit_iterations: accepted Gauss-Newton steps. */
typedef struct dsdtm_homography_result {
    double H[9];
    double cost_before, cost_after;
    int32_t found, n_inliers, best_hypothesis, rounds, refit_iterations, reserved;
} dsdtm_homography_result;

/* n independent problems (0 <= n <= DSDTM_HOMOGRAPHY_MAX_PROBLEMS; n == 0: DSDTM_OK, nothing done) in ONE submission: one upload from
 * the pinned block, ONE launch (one 256-thread workgroup per problem), one read-back, one wait. Each result is bit-equal to its single
 * call, wherever it stands in the batch. Everything is validated before anything is enqueued, and a failure names the index and the
 * field; all or nothing: after any failure every output is untouched. Inside a stream capture: DSDTM_ERR_INVALID. */
int dsdtm_find_homographies(dsdtm_homography_ctx* ctx, int n, const dsdtm_homography_desc* descs, dsdtm_homography_result* results);
/* One problem with the default parameters. */
int dsdtm_find_homography(dsdtm_homography_ctx* ctx, int m, const float* points_a, const float* points_b, uint8_t* mask,
                          dsdtm_homography_result* result);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_HOMOGRAPHY_H */
