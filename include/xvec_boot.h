/* xvec_boot.h -- C ABI of the bootstrap in libxvec_hip.so: confidence intervals for EER and minDCF from device scores.
 *
 * xvec_eval.h ends in a point estimate.  This unit says how far that estimate moves when the speakers of the test set
 * change: the speaker-level bootstrap.  The groups (speakers) of the trial sides are resampled with replacement, the trial
 * list is re-evaluated under every resample, and the caller takes percentiles of the n_boot results.  Two systems evaluated
 * with the same seed and groups see the same resamples, which is the paired bootstrap.
 *
 * A resample changes the WEIGHT of a trial, not the order of the scores: the (key, payload) pairs are sorted once, by the
 * sort of xvec_eval.h with a 32-bit payload, and every replicate is a weighted prefix sum and sweep over that one order.
 *
 * TRIALS.  The forms of xvec_eval.h: a trial list (row_idx / col_idx / is_target), the plain vector (both index arrays NULL,
 * n_rows == 1), or all pairs (xvec_boot_all_pairs).  Trial t of all pairs is the cell t = row * n_cols + col.
 *
 * GROUPS.  row_group [n_rows] and col_group [n_cols] (DEVICE int32, either may be NULL) give the group of every row and column
 * of the matrix; n_row_groups = G_0 and n_col_groups = G_1 in 1 .. XVEC_BOOT_MAX_GROUPS count them (0 where the side is NULL).
 * A trial is tested in this order and counted once: an index outside the matrix (n_bad_index), a skipped diagonal cell, a group
 * id outside [0, G_s) on a side that is given (n_bad_group), a NaN score (n_nan).  Such a trial is left out of everything,
 * the point estimate included; the cell of a trial with a bad index or a bad group is never read.
 *
 * WEIGHTS.  Replicates are numbered b = 1 .. n_boot.  philox is Philox4x32-10 (csrc/philox.h) with the key
 * (seed_lo, seed_hi); MAGIC = XVEC_BOOT_MAGIC ("boot").
 *   Group sides.  For replicate b and side s (0 = rows, 1 = columns), draw j, 0 <= j < G_s, is word j & 3 of
 *       philox(counter = (j >> 2, b, s, MAGIC))
 *   and picks the group (uint64(word) * G_s) >> 32.  c_s,b[g] counts how often g was picked: a multinomial resample of G_s
 *   groups out of G_s.  The map's bias of at most G_s / 2^32 per group belongs to this specification.
 *   Trial t in cell (i, j) weighs  w_b(t) = c_0,b[row_group[i]] * c_1,b[col_group[j]];  a NULL side contributes the factor 1.
 *   joint != 0 (enrolment and test speakers from one pool) needs both sides and G_0 == G_1 and uses the ONE draw of side 0 for
 *   both factors: w_b(t) = c_0,b[row_group[i]] * c_0,b[col_group[j]].
 *   Both sides NULL (the only meaning the plain vector has): every trial is its own unit, with a Poisson(1) weight from word
 *   t & 3 of philox(counter = (t >> 2, b, 2, MAGIC)), t the ORIGINAL trial index:  w_b(t) = #{ i : word >= T_i },
 *   T_i = floor(2^32 P[Poisson(1) <= i]), i = 0 .. XVEC_BOOT_POISSON_TERMS - 1 (the table: csrc/boot_plan.h; it ends where T_i reaches
 *   2^32 - 1, so the largest weight is 13, for the one word 0xffffffff).  This is the POISSON bootstrap: the trials' weights are independent and
 *   the size of a replicate varies around n; it is NOT a resample of fixed size n.
 *
 * PER REPLICATE.  The definitions of xvec_eval.h on the multiset in which trial t occurs w_b(t) times.  P_b and N_b are the
 * weighted counts of targets and non-targets; tp_b(k) and nn_b(k) the weighted counts at or below sorted position k.  A
 * candidate is a position k that ends a run of equal keys AND has tp_b(k) + nn_b(k) > 0 (a threshold below every resampled
 * score is not a threshold of the resample).  EER is the arg-min of |(N_b - nn_b) P_b - tp_b N_b| in 64-bit integers, minDCF
 * the arg-min of c_miss FRR p_target + c_fa FAR (1 - p_target) in fp64, lowest k on ties: the expressions of eval.hip
 * themselves (csrc/trial_device.h).  All counts are integers; tile sums and the scan over tiles run in 64 bits.
 *   A replicate with P_b + N_b >= 2^31 would overflow the cross products: it is counted in n_overflow, its doubles are NaN.
 *   A replicate with P_b == 0 or N_b == 0 is counted in n_degenerate, its doubles are NaN.  (The point estimate is counted in
 *   neither; its n_target / n_nontarget say it.)
 *
 * DETERMINISM.  Replicate b depends on nothing but (seed, b), the groups and the trials: it is bit-identical from call to
 * call, whatever the workspace held, whatever n_boot is and however the replicates were batched.  No float atomics; the only
 * atomics are integer counts, whose order does not matter.
 *
 * Conventions as xvec_eval.h: DEVICE pointers unless said otherwise, asynchronous on the caller's stream, no allocation, return
 * codes as xvec_hip.h (0 = OK) with the message from xvec_boot_last_error().
 */
#ifndef XVEC_BOOT_H
#define XVEC_BOOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_BOOT_MAX_GROUPS 16384
#define XVEC_BOOT_MAX_BOOT 100000
#define XVEC_BOOT_MAGIC 0x626f6f74
#define XVEC_BOOT_POISSON_TERMS 13

/* HOST struct: what a run is drawn with. */
typedef struct {
    const int32_t* row_group; /* DEVICE [n_rows] or NULL */
    const int32_t* col_group; /* DEVICE [n_cols] or NULL */
    int32_t n_row_groups;     /* G_0; 0 iff row_group is NULL */
    int32_t n_col_groups;     /* G_1; 0 iff col_group is NULL */
    int32_t joint;
    int32_t n_boot;           /* 1 .. XVEC_BOOT_MAX_BOOT */
    uint64_t seed;
    double c_miss, c_fa, p_target;
} xvec_boot_params;

/* Written by the device: record 0 is the point estimate (every weight 1; field for field what xvec_eval_trials /
 * xvec_eval_all_pairs write for the same arguments), records 1 .. n_boot the replicates. */
typedef struct {
    double eer;
    double eer_threshold;
    double far;
    double frr;
    double min_dcf;
    double min_dcf_threshold;
    int64_t n_target;    /* P_b */
    int64_t n_nontarget; /* N_b */
} xvec_boot_record;

typedef struct {
    int64_t n_nan;
    int64_t n_bad_index;
    int64_t n_bad_group;
    int64_t n_degenerate;
    int64_t n_overflow;
} xvec_boot_summary;

const char* xvec_boot_last_error(void);

/* Scratch for n_trials trials (n_rows * n_cols for all pairs); 0 for arguments the entry points refuse. */
size_t xvec_boot_workspace_bytes(int64_t n_trials, int32_t n_boot, int32_t n_row_groups, int32_t n_col_groups);

/* Replicates processed per batch and the number of batches (0: refused): functions of (n_trials, n_boot) alone. */
int32_t xvec_boot_batch(int64_t n_trials, int32_t n_boot);
int32_t xvec_boot_batches(int64_t n_trials, int32_t n_boot);

/* records [n_boot + 1], summary: device memory.  Other arguments as xvec_eval_trials. */
int xvec_boot_trials(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                     const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, const xvec_boot_params* params,
                     xvec_boot_summary* summary, xvec_boot_record* records, void* workspace, size_t workspace_bytes,
                     xvec_stream stream);

/* Arguments as xvec_eval_all_pairs. */
int xvec_boot_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                        const int32_t* col_class, int32_t skip_diagonal, const xvec_boot_params* params,
                        xvec_boot_summary* summary, xvec_boot_record* records, void* workspace, size_t workspace_bytes,
                        xvec_stream stream);

/* On the HOST, without a GPU: the count table c_s,b [n_groups] of (seed, b, side), and the Poisson weight of (seed, b, t).
 * Both return 0, or XVEC_ERR_ARG with the message. */
int xvec_boot_counts_host(uint64_t seed, int32_t b, int32_t side, int32_t n_groups, uint16_t* counts_out);
int xvec_boot_poisson_host(uint64_t seed, int32_t b, int64_t t, int32_t* weight_out);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_BOOT_H */
