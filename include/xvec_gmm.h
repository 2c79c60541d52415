/* xvec_gmm.h -- C ABI of the GMM-UBM unit in libxvec_hip.so: diagonal-covariance EM, Baum-Welch statistics, relevance MAP
 * and the scores of the classical GMM-UBM verifier (the i-vector baseline's front half: SIDEKIT's stat0 / stat1).
 *
 * MODEL.  Weights w[C], means mu[C, D], variances v[C, D] (v > 0), DEVICE fp64, 1 <= C <= XVEC_GMM_MAX_C,
 * 1 <= D <= XVEC_GMM_MAX_D.  xvec_gmm_prepare writes the prepared form
 *   P[C, 2D] = (mu / v, -0.5 / v),    g[C] = log w - 0.5 (D log 2 pi + sum_d log v + sum_d mu^2 / v),
 * the sums over d taken in rising d.  w_c = 0 gives g_c = -inf: that component has posterior exactly 0 everywhere, never NaN.
 * With X'[n] = (x_n, x_n^2), the squares taken in fp64 from the widened value, ll[n, c] = g[c] + X'[n] . P[c].
 * This is Kaldi's expanded form: -0.5 (x - mu)^2 / v is computed as three terms that cancel, so ll carries an absolute error
 * of the order of u . sum_d (x_d^2 + mu_d^2) / v_d (u = 2^-53), where the centred form's would be u . |ll|.  With data and
 * means offset by 10, 100 and 1000 standard deviations the fp64 restatement in this form moves by 8e-13, 4e-11 and 5e-9
 * against the centred form; fp32 has 2^29 times less room.  That is why the unit is fp64 throughout.
 *
 * FRAMES (xvec_gmm_frames, a HOST struct).  x is [rows, D] with row stride ldx, DEVICE, fp32 (XVEC_GMM_X_F32) or fp64
 * (XVEC_GMM_X_F64); an fp32 input gives, bit for bit, what its widened fp64 copy gives.  The utterances are HOST arrays
 * utt_first[n_utts], utt_count[n_utts]: every range must lie inside [0, rows); ranges may overlap; a count of 0 is allowed.
 * They are checked on the host and uploaded in stream order (they must stay valid until the call returns).  The FRAMES of a
 * call are the rows of the ranges, utterance after utterance: frame j of n_total = sum of the counts (<= 2^30).  A row
 * that two ranges share is two frames.  Rows outside every range are never read: packed frames, padded [B, T, D] batches
 * (utt_first = b T) and sliding windows are served without a copy, and nothing depends on what padding holds.
 * A frame with a non-finite coefficient, or whose lse is not finite, is BAD: it is left out of every sum and counted once in
 * n_bad.  (A non-finite coefficient always gives a non-finite lse: the test on lse is the one made.)
 *
 * SUMMATION ORDER.  fp64, no float atomics; every sum runs in a fixed order, and results are bit-identical from call to call
 * whatever the workspace held.  ll: K = 2D in rising chunks of 16 on v_mfma_f64_16x16x4_f64.  lse: online (max, sum) over the
 * component tiles of 64 in rising order, four running pairs per frame (components c with (c % 64) / 16 = q), merged q = 0..3.
 * Statistics: the frames of a slice (global form) or of an utterance in rising chunks of 64 on the same MFMA; the slices are
 * then added in rising order.  Sums over frames of lse: thread i of 256 adds the frames i, i + 256, ..; then a fixed tree.
 *
 * M-STEP.  scikit-learn's _estimate_gaussian_parameters for 'diag' and the renormalisation of GaussianMixture._m_step:
 *   nk = n + 10 eps,  w = (nk / n_frames) / sum_c (nk / n_frames),  mu = f / nk,  v = s / nk - mu^2 + reg_covar,
 * then v = max(v, var_floor); a component with n < min_count keeps its mean and variance (its weight is still updated).
 * s / nk - mu^2 cancels where mu^2 >> v: the variance carries a relative error of the order of u (1 + mu^2 / v), so fp64
 * leaves 16 - 2 log10(mu / sigma) digits: ten at an offset of 1000 standard deviations.  Centre such features (CMVN) first.
 *
 * Conventions as xvec_hip.h: DEVICE pointers unless stated (the frames and option structs and utt_* are HOST), asynchronous on
 * the caller's stream, no allocation, return codes as xvec_hip.h with the message from xvec_gmm_last_error().  Arguments are
 * checked, and a null or short workspace refused, before a device is touched.
 *
 * NOT BUILT: the i-vector extractor (total variability matrix) that reads the same statistics, full covariances, k-means
 * initialisation and mixture splitting, delta features.
 */
#ifndef XVEC_GMM_H
#define XVEC_GMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_GMM_MAX_C 4096
#define XVEC_GMM_MAX_D 256
#define XVEC_GMM_MAX_UTTS 16777216
#define XVEC_GMM_MAX_SLICES 1024
#define XVEC_GMM_MAX_ITER 10000
#define XVEC_GMM_FRAME_TILE 64
#define XVEC_GMM_COMP_TILE 64
#define XVEC_GMM_X_F32 0
#define XVEC_GMM_X_F64 1

/* HOST struct. */
typedef struct {
    const void* x;            /* DEVICE [rows, D], row stride ldx >= D */
    int32_t x_type;           /* XVEC_GMM_X_F32 | XVEC_GMM_X_F64 */
    int32_t reserved;         /* 0 */
    int64_t rows;
    int64_t ldx;
    const int64_t* utt_first; /* HOST [n_utts] */
    const int64_t* utt_count; /* HOST [n_utts] */
    int64_t n_utts;           /* 1 .. XVEC_GMM_MAX_UTTS */
} xvec_gmm_frames;

/* HOST struct. */
typedef struct {
    double reg_covar; /* >= 0, added to every variance (scikit-learn's default: 1e-6) */
    double var_floor; /* >= 0, 0 = none */
    double min_count; /* >= 0, 0 = every component is updated */
} xvec_gmm_mstep_options;

const char* xvec_gmm_last_error(void);

/* On the HOST: out[0] frame tile, out[1] component tile, out[2] component tiles, out[3] column tiles of the statistics
 * (1 + 2D columns in the global form, 1 + D per utterance, 64 a tile), out[4] slices (per_utt: 0), out[5] frames per slice,
 * out[6] K = 2D padded to 4, out[7] K chunks of 16, out[8] doubles of the slab, out[9] blocks of the statistics kernel.
 * n_slices = 0: the plan's choice; 1 .. XVEC_GMM_MAX_SLICES forces it.  0, or XVEC_ERR_ARG. */
int xvec_gmm_plan_host(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices, int64_t* out);

/* Scratch; 0 for arguments the entry points refuse. */
size_t xvec_gmm_loglik_workspace_bytes(int64_t n_utts, int32_t C, int32_t D);
size_t xvec_gmm_accumulate_workspace_bytes(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices);
size_t xvec_gmm_em_workspace_bytes(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t n_slices);
size_t xvec_gmm_linear_scores_workspace_bytes(int64_t M, int64_t U, int32_t C, int32_t D);

/* P [C, 2D], g [C] from the model; mu_override (may be NULL) replaces mu. */
int xvec_gmm_prepare(const double* w, const double* mu, const double* v, const double* mu_override, int32_t C, int32_t D, double* P,
                     double* g, xvec_stream stream);

/* lse [n_total]: log sum_c exp(ll[j, c]) of every frame (as computed, also for bad frames); utt_llsum [n_utts], utt_frames
 * [n_utts]: the sum of lse over, and the count of, the good frames of each utterance; n_bad [1]; gamma (may be NULL)
 * [n_total, C]: the posteriors, rows of zeros for bad frames.  mu_override (may be NULL) [C, D]: the same weights and
 * variances with other means -- a MAP-adapted model; the exact LLR against the UBM is two calls and a subtraction. */
int xvec_gmm_loglik(const xvec_gmm_frames* frames, const double* w, const double* mu, const double* v, const double* mu_override,
                    int32_t C, int32_t D, double* lse, double* utt_llsum, int64_t* utt_frames, int64_t* n_bad, double* gamma,
                    void* workspace, size_t workspace_bytes, xvec_stream stream);

/* per_utt == 0, the E-step: n [C] = sum gamma, f [C, D] = sum gamma x, s [C, D] = sum gamma x^2 over all frames; llsum [1],
 * n_frames [1], n_bad [1].
 * per_utt != 0, the Baum-Welch statistics: n [n_utts, C], f [n_utts, C, D] (s is not looked at), llsum [n_utts], n_frames
 * [n_utts], n_bad [1].  An empty utterance gives exact zeros.  n_slices must be 0. */
int xvec_gmm_accumulate(const xvec_gmm_frames* frames, const double* w, const double* mu, const double* v, int32_t C, int32_t D,
                        int32_t per_utt, int32_t n_slices, double* n, double* f, double* s, double* llsum, int64_t* n_frames,
                        int64_t* n_bad, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* New w, mu, v (written in place) from n, f, s and the DEVICE scalar n_frames. */
int xvec_gmm_mstep(const double* n, const double* f, const double* s, const int64_t* n_frames, int32_t C, int32_t D,
                   const xvec_gmm_mstep_options* options, double* w, double* mu, double* v, xvec_stream stream);

/* max_iter iterations of prepare -> accumulate -> M-step on w, mu, v in place, nothing read back.  lower_bound [max_iter]:
 * llsum / n_frames of each iteration's E-step (NaN for iterations not run); the test |lower_bound[it] - lower_bound[it - 1]|
 * < tol (the first iteration compares with -inf) runs on the device after the M-step, as scikit-learn's does, and the later
 * iterations return at once on a device flag.  n_iter_done [1] int32, n_bad [1] (of the last iteration run).  Utterances
 * without a single frame are refused. */
int xvec_gmm_em(const xvec_gmm_frames* frames, int32_t C, int32_t D, int32_t max_iter, double tol,
                const xvec_gmm_mstep_options* options, int32_t n_slices, double* w, double* mu, double* v, double* lower_bound,
                int32_t* n_iter_done, int64_t* n_bad, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* Relevance MAP of the means for M rows of statistics n [M, C], f [M, C, D]: alpha = n / (n + relevance),
 * mu_hat[m, c, :] = alpha f / n + (1 - alpha) mu; n = 0 gives mu exactly, by selection (no 0 / 0).  relevance > 0. */
int xvec_gmm_map_means(const double* n, const double* f, const double* mu, int64_t M, int32_t C, int32_t D, double relevance,
                       double* mu_hat, xvec_stream stream);

/* Glembek's linear scoring: S[m, u] = sum_{c, d} (mu_hat[m, c, d] - mu[c, d]) / v[c, d] . (f[u, c, d] - n[u, c] mu[c, d])
 * / sum_c n[u, c]; a test row with sum_c n = 0 scores exactly 0.  S is [M, U] with row stride ld_s (PldaScorer.score's
 * layout).  Two preparation kernels write the supervectors; a third multiplies them, the sum over K = C D taken in blocks of
 * 32 terms (each block, then the blocks, in rising order). */
int xvec_gmm_linear_scores(const double* mu_hat, int64_t M, const double* n, const double* f, int64_t U, const double* mu,
                           const double* v, int32_t C, int32_t D, double* S, int64_t ld_s, void* workspace, size_t workspace_bytes,
                           xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_GMM_H */
