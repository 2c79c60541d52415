/* xvec_analyze.h -- C ABI of score analysis in libxvec_hip.so: moments, histograms and the hardest trials of device scores.
 *
 * What the reference's extra/compare_speaker_results.py computes once the EER is known: maximum, minimum, mean and variance of
 * all, of the target and of the non-target scores (its lines 47-63), the distributions of the rounded scores (72-96) and the
 * highest-scoring non-target and lowest-scoring target cells (98-150).  Here the scores stay on the device.
 *
 * TRIALS.  The forms are those of xvec_eval.h: a trial list, the plain vector (row_idx == col_idx == NULL, n_rows == 1) and
 * all pairs; n_trials <= 2^31 - 1.  Every trial goes through the reader of xvec_eval_trials: a trial whose score is NaN or whose
 * index lies outside the matrix is counted (n_nan, n_bad_index) and left out of everything else.  The all-pairs forms take
 * skip_diagonal and upper_only: with upper_only != 0 only cells with row < col take part (a self-scored symmetric matrix is
 * counted once per unordered pair); the cells it leaves out are counted nowhere, like the diagonal's.  Trial index t is the
 * position in the list, row * n_cols + col for all pairs.  Class 0 is non-target, class 1 target, "all" (2) their union.
 * Infinite scores are ordinary values: they enter min and max, the under- and overflow slots and the hardest lists; mean and
 * variance then follow IEEE.
 *
 * SUMMARY (xvec_analyze_summary, _all_pairs).  Two passes over the trials.  Pass 1: n, min, max (with the LOWEST trial index
 * that attains each), the sum and, if asked for, the histogram.  mean = sum / n, moved into [min, max] where rounding put it
 * outside.  Pass 2: M2 = sum of (s - mean)^2, var = M2 / n: the population variance (np.var); nothing cancels, n == 1 and
 * equal scores give exactly 0.  An empty class has n = 0, t_min = t_max = -1 and NaN in the four doubles.
 * SUMMATION ORDER.  fp64, no float atomics, bit-identical from call to call whatever the workspace held.  The trials are cut
 * into tiles of XVEC_ANALYZE_TILE; block b of G = min(tiles, XVEC_ANALYZE_MAX_BLOCKS) walks the tiles [b tiles / G,
 * (b + 1) tiles / G) in rising order, thread i adding the trials base + j * 256 + i (j = 0 .. 7) of each to ONE running sum per
 * class; the threads' sums are combined by a butterfly over the wave's lanes (offsets 1, 2, .., 32), the four waves in wave
 * order; one block then adds the blocks' sums: thread i the blocks i, i + 256, ... in rising order, then butterfly and waves again.
 * xvec_analyze_plan_host reports the depth of that tree.  "All" is merged from the classes, class 0 first:
 *   n = n_0 + n_1, sum = sum_0 + sum_1, M2 = (M2_0 + M2_1) + (n_0 (mean_0 - mean)^2 + n_1 (mean_1 - mean)^2);
 * with one class empty it is the other class, bit for bit.
 *
 * HISTOGRAM (bins != NULL).  Score s falls into bin b = R(s / width) - first: one correctly rounded fp64 division, R = floor
 * (XVEC_ANALYZE_FLOOR) or rint, ties to even (XVEC_ANALYZE_RINT).  R(s / width) is compared with first and first + n_bins - 1 as
 * a double, before any conversion to an integer: below goes to slot 0 (underflow), above to slot n_bins + 1 (overflow), bin b to
 * slot b + 1.  counts is int64 [2][n_bins + 2], class 0 first.  width = 1 and RINT is the reference's np.rint(score).  Integer
 * atomics only: LDS tables first (hist_copies private copies per block, 0 = the plan's choice), then global.
 *
 * HARDEST (xvec_analyze_hardest, _all_pairs).  The k highest-scoring non-target trials and the k lowest-scoring target
 * trials, as records in that order (the hardest first).  The order is that of the fp64 value itself (the 64-bit key of
 * csrc/snorm_keys.h; -0.0 and +0.0 are equal), NOT the fp32 rounding xvec_eval sorts by; ties go to the lower t, within a list
 * too.  A class with fewer than k trials gives a short list: counts[0] / counts[1] say how many records the non-target /
 * target list holds, counts[2] = n_nan, counts[3] = n_bad_index.  A radix select: digit passes over the trials (most
 * significant 8 bits first) until the bucket that holds the k-th key, with everything above it, fits cand_cap candidates;
 * an order-preserving compaction into that buffer; the rest of the walk over the candidates; one block orders the survivors.
 * Exact and bit-identical from run to run; the workspace does not grow with n_trials.
 *
 * Conventions as xvec_hip.h: DEVICE pointers (the bins and select structs are HOST), asynchronous on the caller's stream, no
 * allocation, return codes as xvec_hip.h with the message from xvec_analyze_last_error().  Arguments are checked, and a null or
 * short workspace refused, before a device is touched.
 */
#ifndef XVEC_ANALYZE_H
#define XVEC_ANALYZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_ANALYZE_MAX_BINS 4094
#define XVEC_ANALYZE_MAX_K 2048
#define XVEC_ANALYZE_TILE 2048
#define XVEC_ANALYZE_MAX_BLOCKS 1024
#define XVEC_ANALYZE_MAX_CAND 65536
#define XVEC_ANALYZE_FLOOR 0
#define XVEC_ANALYZE_RINT 1

typedef struct {
    int64_t n;
    int64_t t_min; /* the lowest trial index whose score equals min; -1 for an empty class */
    int64_t t_max;
    double min;
    double max;
    double mean;
    double var;
    double sum;    /* the sum the mean was taken from */
} xvec_analyze_class;

/* Written by the device. */
typedef struct {
    xvec_analyze_class cls[3]; /* 0 non-target, 1 target, 2 all */
    int64_t n_nan;
    int64_t n_bad_index;
} xvec_analyze_stats;

/* HOST struct. */
typedef struct {
    double width;        /* > 0 and finite */
    int64_t first;       /* the lattice label of bin 0; |first| <= 2^52 */
    int32_t n_bins;      /* 1 .. XVEC_ANALYZE_MAX_BINS */
    int32_t rounding;    /* XVEC_ANALYZE_FLOOR | XVEC_ANALYZE_RINT */
    int32_t hist_copies; /* 0: the plan's choice; else a power of two up to the plan's maximum for n_bins */
    int32_t reserved;    /* 0 */
} xvec_analyze_bins;

/* HOST struct. */
typedef struct {
    int32_t k;        /* 1 .. XVEC_ANALYZE_MAX_K */
    int32_t cand_cap; /* 0: the plan's default; else k .. XVEC_ANALYZE_MAX_CAND */
} xvec_analyze_select;

typedef struct {
    double score;
    int32_t row;
    int32_t col;
    int64_t t;
} xvec_analyze_record;

const char* xvec_analyze_last_error(void);

/* On the HOST: out[0] tiles, out[1] blocks G, out[2] the most tiles a block walks, out[3] the depth of the summation tree
 * (additions on the longest path from a term to the sum), out[4] the LDS copies of the histogram for n_bins (0 without),
 * out[5] the most copies n_bins allows, out[6] the default cand_cap, out[7] the trial count from which a block walks a
 * second tile.  0, or XVEC_ERR_ARG. */
int xvec_analyze_plan_host(int64_t n_trials, int32_t n_bins, int64_t* out);

/* Scratch; 0 for arguments the entry points refuse.  n_trials = n_rows * n_cols for all pairs. */
size_t xvec_analyze_summary_workspace_bytes(int64_t n_trials, int32_t n_bins);
size_t xvec_analyze_hardest_workspace_bytes(int64_t n_trials, int32_t k, int32_t cand_cap);

/* bins == NULL: no histogram, counts is not looked at.  Other arguments as xvec_eval_trials. */
int xvec_analyze_summary(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                         const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, const xvec_analyze_bins* bins,
                         xvec_analyze_stats* out, int64_t* counts, void* workspace, size_t workspace_bytes,
                         xvec_stream stream);

int xvec_analyze_summary_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                   const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal,
                                   int32_t upper_only, const xvec_analyze_bins* bins, xvec_analyze_stats* out, int64_t* counts,
                                   void* workspace, size_t workspace_bytes, xvec_stream stream);

/* nontarget_out, target_out: [select->k] records each; counts: int64 [4]. */
int xvec_analyze_hardest(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                         const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials,
                         const xvec_analyze_select* select, xvec_analyze_record* nontarget_out,
                         xvec_analyze_record* target_out, int64_t* counts, void* workspace, size_t workspace_bytes,
                         xvec_stream stream);

int xvec_analyze_hardest_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                   const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal,
                                   int32_t upper_only, const xvec_analyze_select* select, xvec_analyze_record* nontarget_out,
                                   xvec_analyze_record* target_out, int64_t* counts, void* workspace, size_t workspace_bytes,
                                   xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_ANALYZE_H */
