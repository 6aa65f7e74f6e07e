/*
 * dsdtm_amd_rarsac.h — C ABI of libdsdtm_amd_rarsac.so: Rarsac_base::RejectFundamental for n trackers in one launch on the MI355X (gfx950).
 *
 * An ADD-ON library beside libdsdtm_amd.so, like libdsdtm_amd_homography.so and libdsdtm_amd_framediff.so: a header, a context and sources
 * of its own. It shares their conventions — POD arguments, caller-owned memory, `int` status returns (the DSDTM_* codes), no exceptions,
 * no globals, no environment, one context per calling thread, NO CPU fallback — and nothing else.
 *
 * Replaces: Rarsac_base (include/Rarsac_base.h, src/Rarsac_base.cpp): the grid-guided RANSAC for the fundamental matrix that rejects
 *           outliers among frame-to-frame correspondences and updates the frame's 10x10 inlier-probability grid
 *           (Frame::mvGrid_probability, Frame::Reset_Gridproba). Tracking owns an instance (include/Tracking.h:127);
 *           Test/test_Optimizer.cpp:91-106 shows its pipeline: pyramidal LK (here: dsdtm_klt_flow), then epipolar outlier rejection.
 *
 * PARITY. OpenCV is not available to this project, in source or binary: cv::SVDecomp and std::random_shuffle cannot be restated, and
 * the reference's sampling loop (src/Rarsac_base.cpp:161-271) reads past mvBinIndexProba and never clears its sample. Therefore WHICH
 * SAMPLES ARE DRAWN AND HOW THE 8-POINT SYSTEM IS SOLVED ARE THIS PROJECT'S DEFINITION (R3, R4); the scoring, the grid update, the
 * best-so-far rule and the stop rule (R5-R8) follow the reference operation by operation. The yardstick is
 * dsdtm_amd/rarsac_restatement.py with its plain-C twin tests/rarsac_restatement.c and the host function of
 * dsdtm_amd/host/dsdtm_rarsac_host.hpp: the three are bit-equal and the device is bit-equal to them in every output. Parity with OpenCV
 * is unpinned and stays unpinned.
 *
 * THE DEFINITION (every decision rests on + - * / sqrt without contraction, in one order of operations; "float" is IEEE binary32):
 *   R1 bins      (:17-20, :90-94) gr = height / 10, gc = width / 10 (integers). THE REFERENCE'S SWAPPED DIVISORS ARE KEPT:
 *                index = (int)(y / gc) * 10 + (int)(x / gr), both divisions in float, of the CURRENT point. A correspondence whose
 *                index falls outside 0..99 (there the reference writes out of bounds; a quotient beyond +-1e6 counts as outside) or
 *                with a coordinate that is not finite: DSDTM_ERR_INVALID naming the problem and the index. Bin centres as in
 *                src/Camera.cpp:70-78: (gr * (j / 10) + gr / 2, gc * (j % 10) + gc / 2), integers.
 *   R2 priors    (:29-37) bin_probability[j] = prior[j] / sum(prior), the sum in index order from 0.0. prior = grid_probability_in,
 *                each in 0..1, with a positive sum.
 *   R3 sampling  (this project's definition; guided by the grid as the reference intends) counter-based with the 32-bit hash of
 *                dsdtm_amd_homography.h. The non-empty bins in bin order carry the integer weights max(1, (int)(prior[j] * 1024)) and
 *                their inclusive prefix sums, W the last. Draw c of hypothesis k picks the first bin whose prefix sum exceeds
 *                (hash(seed, k, c) * W) >> 32; a bin that the sample already holds is redrawn with the next counter; when 64 draws
 *                did not give 8 distinct bins the hypothesis is invalid. Bin s of the sample (s = 0..7, in the order drawn) gives its
 *                correspondence number (hash(seed, k, 64 + s) * a[bin]) >> 32 counted in index order. With fewer than 8 non-empty
 *                bins: found = 0 and NOTHING ELSE is written. Hypothesis k is the same whichever lane or round evaluates it.
 *   R4 solver    (the shape of ComputeF21 and Normalize_Points, :377-457) per image and axis, in double from the widened floats:
 *                mean = sum(x / 8), dev = sum(|x - mean| / 8), scale 1 / dev. The 8x9 system has the reference's column order
 *                (:433-441): u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1 (1 = current, 2 = previous). Its null vector by Gaussian
 *                elimination with COMPLETE PIVOTING, rows and columns keeping their indices (no exchange): among the unused rows and
 *                columns the largest magnitude wins, ties go to the lowest row, then the lowest column; every unused row i takes
 *                A[i][.] - (A[i][pc] / pivot) * A[pr][.]. Back substitution with the free unknown set to 1, each sum over the columns
 *                in index order; then the vector is scaled to unit norm. A final pivot at or below 1e-12 times the largest initial
 *                magnitude, or any value that is not finite, makes the hypothesis invalid. Rank 2: v = the unit eigenvector of
 *                F^T F with the smallest eigenvalue (lowest index among equals) by a cyclic 3x3 Jacobi of 8 sweeps over (0,1), (0,2),
 *                (1,2), a zero off-diagonal entry skipped; F <- F - (F v) v^T. De-normalised as (T2^T F) T1 and narrowed to float32
 *                ONCE (the reference's CV_32F); an entry that is not finite then makes the hypothesis invalid.
 *   R5 scoring   (CheckFundamental, :285-362) in float32 exactly as written: th = 3.841f, invSigmaSquare = 1.0 / (sigma * sigma)
 *                narrowed to float, both point-to-line distances, each tested with chiSquare > th AS WRITTEN, so that a NaN distance
 *                does not reject. a[j] counts every correspondence of bin j, b[j] its inliers.
 *   R6 grid      (:365-372, :212-235) p[j] = max(0.2, (double)b / a), 0.2 for an empty bin. S = sum p, Q = sum p p, the weighted mean
 *                of the bin centres, the 2x2 weighted covariance sum (p d) d^T scaled as (C * S) / (S * S - Q),
 *                score = (S * M_PI) * sqrt(det), all in the reference's order of operations.
 *   R7 best      (:238-251) hypotheses in index order; one wins when score > best is strictly true, best starting at DBL_MIN: a
 *                score of 0 never wins and neither does NaN. On a win the status and the grid become the result's, since_best = 0
 *                and q = 1 - t^8 with t = sum p[j] * bin_probability[j], the power by three squarings.
 *   R8 stop      (:253-262) after every VALID hypothesis since_best++ and err = (float)(q^since_best), a running product in double;
 *                the run stops at the first hypothesis with err < terminate_threshold. Invalid hypotheses count against
 *                max_iterations and take no part in R7 or R8. QUIRK: q is 0 before the first win, so a first valid hypothesis that does
 *                not win stops the run — found = 1, best_hypothesis = -1, the status all zero, F zero, the grid the prior, score
 *                DBL_MIN. The same is returned when every hypothesis was invalid (iterations_run = max_iterations).
 *   R9 order     the device evaluates hypotheses in rounds of 256 (lane = hypothesis) and resolves the winner and the stop index by
 *                an ordered scan over the round's scores: the result is that of the sequential evaluation in index order, bit for
 *                bit, and does not depend on a problem's place in a batch.
 */
#ifndef DSDTM_AMD_RARSAC_H
#define DSDTM_AMD_RARSAC_H

#include "dsdtm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSDTM_RARSAC_GRID 100
#define DSDTM_RARSAC_MIN_POINTS 8
#define DSDTM_RARSAC_MAX_POINTS 2048
#define DSDTM_RARSAC_MAX_PROBLEMS 1024
#define DSDTM_RARSAC_MAX_ITERATIONS 16384
#define DSDTM_RARSAC_DEFAULT_ITERATIONS 1000
#define DSDTM_RARSAC_DEFAULT_TERMINATE 0.001
#define DSDTM_RARSAC_DEFAULT_SIGMA 0.5
#define DSDTM_RARSAC_DEFAULT_SEED 0x2545F491u
#define DSDTM_RARSAC_MIN_SIDE 10
#define DSDTM_RARSAC_MAX_SIDE 16384

typedef struct dsdtm_rarsac_ctx dsdtm_rarsac_ctx;
/* device = HIP device ordinal. Fails with DSDTM_ERR_NO_DEVICE when no gfx950 device is usable. */
int dsdtm_rarsac_create(int device, dsdtm_rarsac_ctx** out);
void dsdtm_rarsac_destroy(dsdtm_rarsac_ctx* ctx);
/* Last error text of this context (or of the failed dsdtm_rarsac_create when ctx == NULL). */
const char* dsdtm_rarsac_last_error(const dsdtm_rarsac_ctx* ctx);

/* One problem. cur / prev: m x 2 floats (x, y) in host memory, DSDTM_RARSAC_MIN_POINTS <= m <= DSDTM_RARSAC_MAX_POINTS. status: m bytes in
 * host memory or NULL (not wanted). F: 9 floats, row-major, read by dsdtm_rarsac_check only. grid_probability_in: the frame's prior
 * (Reset_Gridproba gives 0.5 everywhere); dsdtm_rarsac_check does not read it. max_iterations, terminate_threshold, sigma and seed: 0
 * means the default above; max_iterations at most DSDTM_RARSAC_MAX_ITERATIONS. */
typedef struct dsdtm_rarsac_desc {
    const float* cur;
    const float* prev;
    uint8_t* status;
    const float* F;
    double grid_probability_in[DSDTM_RARSAC_GRID];
    double terminate_threshold;
    float sigma;
    uint32_t seed;
    int32_t m, width, height, max_iterations;
} dsdtm_rarsac_desc;

/* found = 0: no other field is written (and no byte of the status). F: the winning matrix, x_prev^T F x_cur = 0. */
typedef struct dsdtm_rarsac_result {
    double grid_probability_out[DSDTM_RARSAC_GRID];
    double score;
    float F[9];
    int32_t found, best_hypothesis, iterations_run, n_inliers, reserved[3];
} dsdtm_rarsac_result;

/* n independent problems (0 <= n <= DSDTM_RARSAC_MAX_PROBLEMS; n == 0: DSDTM_OK, nothing done) in ONE submission: one upload from the
 * pinned block, ONE launch (one 256-thread workgroup per problem), one read-back, one wait. Each result is bit-equal to its single call,
 * wherever it stands in the batch. Everything is validated before anything is enqueued, and a failure names the problem and the field;
 * all or nothing: after any failure every output is untouched. Inside a stream capture: DSDTM_ERR_INVALID. */
int dsdtm_rarsac_reject_batch(dsdtm_rarsac_ctx* ctx, int n, const dsdtm_rarsac_desc* descs, dsdtm_rarsac_result* results);
/* One problem with the default parameters. grid_probability_in: 100 doubles, or NULL for 0.5 everywhere. */
int dsdtm_rarsac_reject(dsdtm_rarsac_ctx* ctx, int m, const float* cur, const float* prev, int width, int height, const double* grid_probability_in,
                        uint8_t* status, dsdtm_rarsac_result* result);
/* R5-R6 alone for the caller's descs[t].F — the stateless CheckFundamental: status, n_inliers, grid_probability_out and score of that F
 * (found = 1, best_hypothesis = -1, iterations_run = 0, F copied). The same checks, the same submission, the same atomicity. */
int dsdtm_rarsac_check(dsdtm_rarsac_ctx* ctx, int n, const dsdtm_rarsac_desc* descs_with_F, dsdtm_rarsac_result* results);

#ifdef __cplusplus
}
#endif
#endif /* DSDTM_AMD_RARSAC_H */
