/* xvec_vbx.h -- C ABI of diarization's refinement step in libxvec_hip.so: VBx (Landini et al.), a Bayesian HMM over the
 * x-vectors of a recording whose states are speakers, run by variational Bayes from an initial assignment (the labels that
 * xvec_ahc_cluster of xvec_diar.h left).
 *
 * The reference has no diarization and the VBx package is not a dependency: the text below is the specification, the oracle
 * is its numpy restatement (tests/vbx_ref.py, a log-domain form and the scaled form the kernel runs, each also in extended
 * precision); parity with the VBx package itself is UNPINNED.
 *
 * Input, per recording r (rows rec_start[r] .. rec_start[r + 1] - 1 of X and gamma, T of them): X [T, dim] fp64 with row
 * stride ldx -- x-vectors already projected so that the within-speaker covariance is I and the between-speaker covariance is
 * diag(phi); phi [dim] > 0; responsibilities gamma [T, n_spk] with row stride ldg and speaker priors pi [n_rec, n_spk] (dense),
 * both in/out.  X and phi are not modified.
 *
 * Constants: rho = X * sqrt(phi), G_t = -0.5 * (sum_d X_td^2 + dim * log(2 pi)).  Iteration k = 0 .. max_iter - 1:
 *   1. N_s = sum_t gamma_ts;  invL_sd = 1 / (1 + Fa/Fb * N_s * phi_d);  alpha_sd = Fa/Fb * invL_sd * sum_t gamma_ts rho_td
 *   2. logp_ts = Fa * (sum_d rho_td alpha_sd - 0.5 * sum_d (invL_sd + alpha_sd^2) phi_d + G_t)
 *   3. forward-backward with tr_ij = loop_prob * [i == j] + (1 - loop_prob) * pi_j from the initial distribution pi, in the
 *      scaled form: b_t = exp(logp_t - max_t), v_0 = pi * b_0, v_tj = (loop_prob * a_{t-1,j} + (1 - loop_prob) * pi_j) * b_tj,
 *      c_t = sum_j v_tj, a_t = v_t / c_t; backwards beta_{T-1} = 1, w_t = b_t * beta_t,
 *      beta_{t-1,j} = (loop_prob * w_tj + (1 - loop_prob) * sum_i pi_i w_ti) / c_t; gamma_t = a_t * beta_t;
 *      tll = sum_t (log c_t + max_t);  pi'_j = gamma_0j + sum_{t >= 1} (1 - loop_prob) * pi_j * w_tj / c_t (the posterior of
 *      arriving in j at t by the non-loop path), then pi' / sum_j pi'_j
 *   4. ELBO_k = tll + Fb * 0.5 * sum_sd (log invL_sd - invL_sd - alpha_sd^2 + 1)
 *   5. stop after iteration k >= 1 if ELBO_k - ELBO_{k-1} < epsilon (epsilon = -inf never stops early)
 * gamma and pi are those of the last iteration run.
 *
 * Rules.  A speaker with pi_j == 0 on entry to an iteration is dead: its gamma column is exactly 0 from then on and it is
 * left out of the row maximum max_t.  labels_t = argmax_s gamma_ts, ties to the lowest s, renumbered per recording in the
 * order of first appearance (the canonical labelling of xvec_ahc_cluster); n_speakers[r] = the number of distinct labels.
 * elbo is [n_rec, max_iter] with NaN in the slots of iterations not run, iters[r] the number run.  A recording whose X, phi,
 * gamma or pi holds a non-finite value (or a phi_d <= 0) gets NaN gamma / pi / elbo, label -1, iters 0 and n_speakers 0 and
 * never affects another recording.  The result is a pure function of the recording's own inputs: bit-identical from run to
 * run and whatever ldx, ldg, the base alignment (8 bytes is all that is asked), the workspace's contents, n_rec or the
 * recording's place in the batch are.  Sums run in a fixed order; no float atomics.
 *
 * One launch per call, one block of XVEC_VBX_THREADS threads per recording, persistent over ALL iterations: the stop test
 * runs on the device and nothing is read back.  Every loop's trip count is fixed by the arguments at launch, no block waits
 * on another.  The two products of an iteration run on v_mfma_f64_16x16x4_f64; one wave walks the two recurrences with a lane
 * per speaker, the rows of b prefetched XVEC_VBX_PREFETCH frames ahead.
 *
 * Conventions as xvec_diar.h: DEVICE pointers (but rec_start_host: a HOST array, checked there and copied into the workspace
 * on the stream), asynchronous on the caller's stream, no allocation (the caller passes a workspace of the queried size),
 * return codes as xvec_hip.h (0 = OK) with the message from xvec_vbx_last_error().
 */
#ifndef XVEC_VBX_H
#define XVEC_VBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* speakers (HMM states) at most: a lane of the recurrence's wave each */
#define XVEC_VBX_MAX_SPEAKERS 64
/* dimension of the projected x-vectors at most */
#define XVEC_VBX_MAX_DIM 512
/* frames (windows) of one recording at most */
#define XVEC_VBX_MAX_FRAMES 16384
/* threads of a recording's block */
#define XVEC_VBX_THREADS 256
/* frames whose rows the recurrence's wave loads ahead of the one it works on */
#define XVEC_VBX_PREFETCH 8

typedef struct {
    double loop_prob; /* in [0, 1) */
    double Fa;        /* > 0 */
    double Fb;        /* > 0 */
    double epsilon;   /* not NaN; -inf never stops early */
    int32_t max_iter; /* >= 1 */
    int32_t reserved; /* 0 */
} xvec_vbx_options;

const char* xvec_vbx_last_error(void);

/* Bytes of workspace for xvec_vbx_run on these recordings (0 for arguments that are refused). */
size_t xvec_vbx_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec, int32_t dim, int32_t n_spk);

/* The initial assignment from labels [N] int32 (N = rec_start_host[n_rec]): row t of gamma is softmax(smoothing * onehot(label_t)),
 * that is e / (e + (n_spk - 1)) at the label and 1 / (e + (n_spk - 1)) elsewhere with e = exp(smoothing) taken on the host;
 * a label outside 0 .. n_spk - 1 gives the uniform row 1 / n_spk.  pi [n_rec, n_spk] is uniform.  One launch. */
int xvec_vbx_init(const int32_t* labels, const int64_t* rec_start_host, int32_t n_rec, int32_t n_spk, double smoothing,
                  double* gamma, int64_t ldg, double* pi, xvec_stream stream);

/* rec_start_host: n_rec + 1 HOST offsets from 0, every recording with 1 .. XVEC_VBX_MAX_FRAMES frames, fewer than 2^31 in all.
 * 1 <= dim <= XVEC_VBX_MAX_DIM, ldx >= dim; 1 <= n_spk <= XVEC_VBX_MAX_SPEAKERS, ldg >= n_spk.  elbo [n_rec, max_iter] fp64, iters [n_rec]
 * int32; labels [N] and n_speakers [n_rec] int32, each may be NULL. */
int xvec_vbx_run(const double* X, int64_t ldx, int32_t dim, const double* phi, const int64_t* rec_start_host, int32_t n_rec,
                 int32_t n_spk, const xvec_vbx_options* options, double* gamma, int64_t ldg, double* pi, double* elbo,
                 int32_t* iters, int32_t* labels, int32_t* n_speakers, void* workspace, size_t workspace_bytes,
                 xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_VBX_H */
