/* xvec_report.h -- C ABI of the trial report in libxvec_hip.so: the score-matrix images and the DET curve.
 *
 * The last stage of the reference (plda_score_stat.py:132-192, the image half of plot_images): the score matrix, the trial
 * masks and the two thresholds become six TensorBoard images.  In numpy each is a [3, N, 2N+5] float64 array; here the score
 * matrix stays on the device and the images are written there, as uint8 or float32.  Four steps:
 *   xvec_report_trial_map   the trial list as a byte map of the matrix: bit 0 of a cell is set if a target trial names it,
 *                           bit 1 if a non-target trial does (the reference's positive_scores_mask / negative_scores_mask,
 *                           which are SET to 1, not counted).  P = bit 0, Ng = bit 1, K = P + Ng (0, 1 or 2);
 *   xvec_report_range       minimum and maximum of the finite cells, and the count of the others;
 *   xvec_report_images      one pass over the matrix and the map that writes every image selected by `which`;
 *   xvec_report_det         the whole error-rate curve (one point per distinct fp32 score) from the sorted keys of
 *                           include/xvec_eval.h, optionally thinned to a grid.
 *
 * DEVIATION from the reference, range: numpy's min / max turn the whole image to NaN on one NaN cell; here the non-finite
 * cells are left out of the range (and counted).  The normalised value of a cell is
 *   v = (S - mn) / (mx - mn)   in fp64: a subtraction, fl(mx - mn), a division;
 * by monotone rounding max(S - mn) = fl(mx - mn), so this is the reference's in-place `-= min; /= max` bit for bit.  A constant
 * matrix gives 0 / 0 = NaN in every cell, as numpy does; a non-finite cell keeps what IEEE 754 makes of it.
 *
 * IMAGES.  With cv = K * S (an fp64 product: the reference multiplies map by score), and for a threshold t
 *   pp_t = [cv >= t] * K,   pn_t = [cv < t] * K    (both 0 where K = 0 and where cv is NaN),
 * the images are, channel by channel (R = n_rows, C = n_cols),
 *   score_matrix                    [R, C] ONE plane   v                 (the reference repeats it in three channels)
 *   ground_truth                    [3, R, C]          Ng       P        0
 *   ground_truth_scores             [3, R, C]          v * Ng   v * P    0
 *   prediction_eer_min_dcf          [3, R, 2C + 5]     pn       pp       0
 *   correct_prediction_eer_min_dcf  [3, R, 2C + 5]     pn * Ng  pp * P   0
 *   false_prediction_eer_min_dcf    [3, R, 2C + 5]     pn * P   pp * Ng  0
 * The three wide images hold the panel of eer_threshold in the columns [0, C), 1 in all three channels in the columns
 * [C, C + 5), and the panel of min_dcf_threshold in the columns [C + 5, 2C + 5).  Every image is contiguous.
 * Two output types:
 *   XVEC_REPORT_F32   the fp64 value rounded once (a cell with K = 2 keeps the value 2);
 *   XVEC_REPORT_U8    trunc(clamp(float32(x) * 255.0f, 0, 255)), NaN -> 0: what torch's TensorBoard writer makes of a float
 *                     image, restated from memory -- torch.utils.tensorboard is not installed where this was written, so
 *                     parity with it is UNPINNED.
 * A block stages a tile of XVEC_REPORT_TILE cells (consecutive columns of one row, or whole rows of a narrow matrix) in LDS
 * -- every cell of the matrix and of the map is read once, with consecutive lanes on consecutive cells -- and writes every
 * selected plane from there in aligned 16-byte pieces; the ragged ends of a row's piece are written element by element.  The
 * uint8 outputs may start at any byte; the float32 outputs must be 4-byte aligned.
 *
 * DET.  The scores are rounded to fp32 and keyed as include/xvec_eval.h keys them (xvec_eval_sorted_keys does it).  For every
 * distinct score u_k in ascending order: thr[k] = u_k, tp[k] = targets <= u_k, nn[k] = non-targets <= u_k, so that
 *   FRR_k = tp[k] / P,   FAR_k = (N - nn[k]) / N     exactly as xvec_eval.h reads them.
 * A flag pass marks the last trial of every run of equal keys, a scan in a fixed order numbers the runs (blocks of
 * XVEC_REPORT_DET_TILE trials, XVEC_REPORT_DET_ITEMS consecutive trials per thread), a compaction writes the points.  With
 * grid = G > 0 the curve is thinned, in 64-bit integers: the first and the last point are kept, and every point at which
 * floor(tp G / P) or floor((N - nn) G / N) differs from its value at the previous distinct score (a quotient by P = 0 or
 * N = 0 counts as 0); both are monotone with at most G steps, so at most 2G + 2 points are left.  grid = 0 keeps every point.
 * A NaN score or an index outside the matrix is counted (n_nan, n_bad_index) and left out, as xvec_eval.h does; the cell
 * of a bad index is never read.  The all-pairs form counts no bad index and leaves a skipped diagonal out silently.
 *
 * Conventions as xvec_hip.h: DEVICE pointers, asynchronous on the caller's stream, no allocation (the caller passes a
 * workspace of the queried size), return codes as xvec_hip.h (0 = OK) with the message from xvec_report_last_error().  No
 * float atomics (integer OR / add only, whose result does not depend on order), every reduction in a fixed order: repeat
 * calls give bit-identical outputs, whatever the workspace held before.
 */
#ifndef XVEC_REPORT_H
#define XVEC_REPORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_REPORT_THREADS 256        /* threads of every block of this unit */
#define XVEC_REPORT_TILE 4096          /* cells a block of the image pass stages */
#define XVEC_REPORT_RANGE_BLOCKS 1024  /* the range pass never launches more: one block reduces the partials */
#define XVEC_REPORT_DET_ITEMS 16       /* consecutive trials a thread scans */
#define XVEC_REPORT_DET_TILE 4096      /* trials a block scans: THREADS * DET_ITEMS */
#define XVEC_REPORT_GAP 5              /* columns of 1 between the two panels of a wide image */

#define XVEC_REPORT_U8 0
#define XVEC_REPORT_F32 1

#define XVEC_REPORT_SCORE_MATRIX 1
#define XVEC_REPORT_GROUND_TRUTH 2
#define XVEC_REPORT_GROUND_TRUTH_SCORES 4
#define XVEC_REPORT_PREDICTION 8
#define XVEC_REPORT_CORRECT 16
#define XVEC_REPORT_FALSE 32
#define XVEC_REPORT_ALL 63

/* Written by the device.  With no finite cell: min = +inf, max = -inf. */
typedef struct {
    double min;
    double max;
    int64_t n_nonfinite;
} xvec_report_range_result;

/* Written by the device.  n_points is the full count, whatever the capacity of the point arrays. */
typedef struct {
    int64_t n_points;
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_nan;
    int64_t n_bad_index;
} xvec_report_det_header;

const char* xvec_report_last_error(void);

/* map[i * ld_map + j] for the [n_rows, n_cols] matrix; zeroed by the call (all n_rows * ld_map bytes), then bit 0 / bit 1
 * set for every trial (arguments as xvec_eval_trials; n_trials may be 0, the three arrays null then).  The bits are set with
 * 32-bit OR atomics on the aligned word that holds the byte: map must be 4-byte aligned and ld_map a multiple of 4 (>= n_cols).
 * A trial with an index outside the matrix is counted in *n_bad_index (device, may be null) and touches no cell. */
int xvec_report_trial_map(const int32_t* row_idx, const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials,
                          int64_t n_rows, int64_t n_cols, uint8_t* map, int64_t ld_map, int64_t* n_bad_index,
                          xvec_stream stream);

/* Scratch of xvec_report_range (it does not depend on the matrix). */
size_t xvec_report_range_workspace_bytes(void);

/* A tile is 4 THREADS consecutive columns of one row, numbered row by row; block b of G = min(tiles, RANGE_BLOCKS) takes the
 * tiles b, b + G, ...; the block's threads combine as a butterfly over the lanes and then in wave order; one block combines
 * the G partials the same way. */
int xvec_report_range(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, xvec_report_range_result* out,
                      void* workspace, size_t workspace_bytes, xvec_stream stream);

/* `range` is the DEVICE record xvec_report_range left.  `which` selects the images (XVEC_REPORT_*, at least one); the
 * pointer of an image that is not selected is ignored and may be null.  dtype: XVEC_REPORT_U8 or XVEC_REPORT_F32.  The
 * outputs must not overlap the inputs or each other.  n_rows * (2 n_cols + 5) <= 2^56. */
int xvec_report_images(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const uint8_t* map, int64_t ld_map,
                       const xvec_report_range_result* range, double eer_threshold, double min_dcf_threshold, uint32_t which,
                       int32_t dtype, void* score_matrix, void* ground_truth, void* ground_truth_scores, void* prediction,
                       void* correct_prediction, void* false_prediction, xvec_stream stream);

/* Scratch for the curve of n_trials trials (0 for a count the calls refuse); n_trials = n_rows * n_cols for all pairs.  One
 * size serves both forms and every grid: beside the sort's window and the sorted pairs (5 n bytes) it always holds the
 * all-pairs trial list (9 n) and the unthinned points (12 n), which a plain list at grid 0 does not use -- about 36 bytes per
 * trial in all. */
size_t xvec_report_det_workspace_bytes(int64_t n_trials);

/* The curve of a trial list (arguments as xvec_eval_trials).  Point k < min(n_points, capacity) goes to thr[k], tp[k],
 * nn[k]; the arrays may be null when capacity == 0.  0 <= grid <= 2^31 - 1. */
int xvec_report_det(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                    const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, int64_t grid,
                    xvec_report_det_header* header, float* thr, int64_t* tp, int64_t* nn, int64_t capacity, void* workspace,
                    size_t workspace_bytes, xvec_stream stream);

/* The curve of every cell (arguments as xvec_eval_all_pairs). */
int xvec_report_det_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                              const int32_t* col_class, int32_t skip_diagonal, int64_t grid, xvec_report_det_header* header,
                              float* thr, int64_t* tp, int64_t* nn, int64_t capacity, void* workspace, size_t workspace_bytes,
                              xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_REPORT_H */
