/* xvec_train.h -- C ABI of a training step in libxvec_hip.so.
 *
 * One frame-level layer of the reference (tdnn_layer.py:26-41) as its training loop runs it (main.py:97-101 under
 * model.train()): context gather, Linear, ReLU and BatchNorm1d on the BATCH statistics, forward and backward
 * (xvec_tdnn_train_*, csrc/tdnn_train.hip).  The five frame-level layers are 99.7 % of a training step's arithmetic.  The
 * tail of the step -- statistics pooling, the three segment-level Linear layers, the cross-entropy loss -- forward and
 * backward, and the Adam update (xvec_train_tail_*, xvec_adam_step, csrc/train_tail.hip): 0.3 % of the arithmetic, but
 * several passes over the layer-5 output and a string of small launches when left to torch ops.  xvector_amd.train uses
 * the tail calls with XVectorTrainer(model, tail="hip").
 *
 * Conventions as xvec_plda.h: stateless (no handle), DEVICE pointers unless the name ends in _host, row-major, fp32,
 * asynchronous on the caller's stream, no allocation (the caller passes a workspace of the queried size), return codes
 * as xvec_hip.h (0 = OK) with the message from xvec_train_last_error().  Every sum runs in a fixed order with no float
 * atomics: repeat calls on the same inputs give bit-identical outputs.  All arithmetic is fp32; the three matrix
 * products run on v_mfma_f32_32x32x2_f32.
 *
 * Shapes.  x [B, T, Cin]; `context_host` holds n_ctx strictly increasing frame offsets (1 <= n_ctx <= 8); with
 * span = context[n_ctx-1] - context[0], T' = T - span and N = B * T'.  Output frame p of an utterance reads the input
 * frames p + context[i] - context[0].  W [Cout, n_ctx * Cin] is torch's own nn.Linear layout over the reference's
 * torch.cat(x_context, 2): column i * Cin + c multiplies channel c of tap i.  It is read as it is on every call (weights
 * change every step: there is no packed copy to keep in step).  B * T < 2^31 and n_ctx * max(Cin, Cout) < 2^31
 * (XVEC_ERR_TOO_LARGE otherwise).
 *
 * Ragged batches (the *_ragged calls; csrc/tdnn_train_ragged.hip, csrc/train_tail_ragged.hip).  The padded layout stays:
 * x [B, T, Cin] with `lengths_dev`, a DEVICE int32 [B] of valid INPUT frames per utterance for that call (as xvec_stat_pool's
 * lengths_dev).  Everything that depends on the lengths is computed on the device -- the valid row count, the row masks, the
 * pooled counts: there is no read-back, no synchronisation and no allocation, and the workspace queries serve both forms
 * unchanged.  The calls compute exactly what the valid frames alone would give.  For a layer with context span s and input
 * lengths l[b], s + 1 <= l[b] <= T:
 *   - utterance b has v[b] = l[b] - s valid output frames, the first v[b] of its T' rows; N = sum of v[b];
 *   - forward: z, batch_mean, batch_var (biased) and y on the valid rows are those of the layer in training mode run on the N
 *     valid rows as ONE BatchNorm batch; every invalid row of z and of y is written as exactly 0.0f.  (A caller that keeps
 *     running statistics moves them with N: the unbiased factor is N / (N - 1).)  The next layer's lengths are l[b] - s;
 *   - backward: dy on invalid rows is ignored, whatever it holds; dgamma, dbeta, dbias and dW sum over the valid rows only, the
 *     1 / N of dz is the valid N, dz is 0 on invalid rows; dx[b, q] receives taps from valid rows only and is exactly 0 for
 *     q >= l[b];
 *   - no result depends on the padding of x or dy, NaN and Inf included: invalid rows are masked by SELECTION on the operands
 *     (they are not loaded), never by a multiplication with 0;
 *   - the tail pools over the v5[b] >= 2 valid frames of utterance b only (mean, unbiased std with divisor v5[b] - 1, a channel
 *     that is constant over them has an std of exactly 0); dy5 on invalid rows is exactly 0; the loss stays the mean over the B
 *     utterances.
 * A length outside its range (a layer: [s + 1, T]; the tail: [2, Tp]) cannot be checked on the host.  Such an utterance
 * contributes no rows: its rows of z, y, dz, dx and dy5 are 0, its pooled row is 0 (it still has a row of logits and a term in
 * the loss); nothing is read or written out of bounds through it.  With no valid row at all batch_mean is 0 and batch_var is NaN (0 / 0).
 * The calls without lengths are these with every length T; their results and code are unchanged by the masked form, which is a
 * compile-time variant of the same kernels.  Two runs of one ragged call are bit-identical.
 *
 * Dropout (the *_dropout calls; csrc/tdnn_train_dropout.hip, csrc/dropout_mask.h).  The reference's layer is Linear, ReLU,
 * Dropout, BatchNorm.  The mask is a stateless function of (seed, stream, row, channel, p): nothing is stored and no generator
 * state lives anywhere.  With n = b * T' + t the row of the padded layout and c the output channel, element (n, c) is decided by
 * word n & 3 of Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) on
 *     counter = (c, n >> 2, low word of stream, high word of stream),   key = (low word of seed, high word of seed):
 *   - the element is DROPPED iff word < thr, thr = (uint32) floor((double) p * 2^32); p = 0 drops nothing;
 *   - forward: z = kept ? max(x_ctx W^T + bias, 0) * scale : 0 with scale = (float) (1 / (1 - (double) p)), one fp32 multiply.
 *     The z that is written (and saved for the backward) is this post-dropout value; batch_mean, batch_var and y are those of
 *     that z, so a caller's running statistics see the post-dropout batch, as torch's do;
 *   - backward: a kept element with a positive pre-activation has z > 0 (scale >= 1), every other one has z == 0 and no
 *     gradient, so dz = [z > 0] scale (the dz of the formulas below): the call needs p, and neither the seed nor a mask;
 *     dgamma and dbeta are the formulas below on the post-dropout z;
 *   - the mask of (n, c) does not depend on B, on the other utterances' lengths or on whether the call is ragged: a ragged
 *     call uses the padded row index, and its invalid rows stay exactly 0;
 *   - 0 <= p < 1, anything else (NaN included) is XVEC_ERR_ARG before any launch.  With p = 0 the calls are bit-identical to
 *     the ones without dropout; two runs of one call are bit-identical.
 */
#ifndef XVEC_TRAIN_H
#define XVEC_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

const char* xvec_train_last_error(void);

/* Scratch of xvec_tdnn_train_forward and xvec_tdnn_train_backward, one size for both (0 for arguments they would
 * refuse). */
size_t xvec_tdnn_train_workspace_bytes(int32_t B, int32_t T, int32_t Cin, int32_t Cout, const int32_t* context_host,
                                       int32_t n_ctx);

/*   z [B, T', Cout]   = ReLU(x_ctx W^T + bias)                      (saved for the backward)
 *   batch_mean [Cout] = mean of z over the N rows
 *   batch_var [Cout]  = BIASED variance of z over the N rows (sums of deviations about a pivot per 256-row chunk,
 *                       merged in chunk order: it survives mean^2 >> var)
 *   y [B, T', Cout]   = gamma (z - batch_mean) / sqrt(batch_var + eps) + beta
 * gamma == NULL: the layer has no BatchNorm; beta, batch_mean, batch_var and y are not touched (y is z). */
int xvec_tdnn_train_forward(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                            int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                            const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                            void* workspace, size_t workspace_bytes, xvec_stream stream);

/* With x^ = (z - batch_mean) / sqrt(batch_var + eps):
 *   dbeta [Cout]             = sum over rows of dy
 *   dgamma [Cout]            = sum over rows of dy x^
 *   dz                       = [z > 0] gamma / sqrt(batch_var + eps) (dy - dbeta / N - x^ dgamma / N)
 *   dbias [Cout]             = sum over rows of dz
 *   dW [Cout, n_ctx * Cin]   = dz^T x_ctx        (rows split into slices, partial products summed in slice order)
 *   dx [B, T, Cin]           : dx[b, q] = sum over taps i of dz[b, q - (context[i] - context[0])] W[:, tap i]; frames
 *                              near an utterance's ends receive fewer taps, none crosses an utterance.  May be NULL.
 * gamma == NULL: no BatchNorm, dz = [z > 0] dy; batch_mean, batch_var, dgamma and dbeta are not touched. */
int xvec_tdnn_train_backward(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                             const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                             const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                             float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                             size_t workspace_bytes, xvec_stream stream);

/* The two calls above over a ragged batch (see the head of this file): the same arguments, plus the device lengths. */
int xvec_tdnn_train_forward_ragged(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                                   int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                                   const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                                   void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev);
int xvec_tdnn_train_backward_ragged(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                                    const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                                    const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                                    float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                    size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev);

/* The same two calls with dropout after the ReLU (see the head of this file).  lengths_dev == NULL: the fixed-length form;
 * otherwise the ragged one.  xvec_tdnn_train_workspace_bytes serves them unchanged.  `dropout_stream` tells the masks of one
 * seed apart (xvector_amd.train: 8 * step + layer); it is not a device stream. */
int xvec_tdnn_train_forward_dropout(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                                    int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                                    const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                                    void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev,
                                    float p, uint64_t seed, uint64_t dropout_stream);
int xvec_tdnn_train_backward_dropout(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                                     const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                                     const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                                     float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                     size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev, float p);

/* keep_host[n * Cout + c] = 1 if element (n, c) is kept, 0 if it is dropped, for n < N: the forward call's own mask, computed
 * on the CPU from the same header (to reproduce a step, and for the tests).  HOST memory; touches no device.  1 <= N < 2^31. */
int xvec_dropout_keep_host(uint8_t* keep_host, int64_t N, int32_t Cout, float p, uint64_t seed, uint64_t dropout_stream);

/* ---- the tail of the step.  C = layer-5 width, Tp = pooled frames (>= 2), H = x-vector size, K = classes; B <= 65535.
 *
 * Scratch of xvec_train_tail_forward and xvec_train_tail_backward, one size for both (0 for arguments they would refuse). */
size_t xvec_train_tail_workspace_bytes(int32_t B, int32_t Tp, int32_t C, int32_t H, int32_t K);

/*   pooled [B, 2C] = (mean over Tp, UNBIASED std over Tp) per utterance and channel, in one pass over y5 [B, Tp, C] as sums
 *                    of deviations about the utterance's first frame: it survives mean^2 >> var, and a channel that is
 *                    constant over the utterance has an std of exactly 0
 *   a6 [B, H]      = ReLU(pooled W6^T + b6)        W6 [H, 2C]   (the reduction split into slices, summed in slice order)
 *   a7 [B, H]      = ReLU(a6 W7^T + b7)            W7 [H, H]
 *   logits [B, K]  = a7 Wo^T + bo                  Wo [K, H]
 *   loss [1]       = mean over the batch, in index order, of logsumexp(logits_b) - logits_b[labels_b]
 * labels: int64 [B] on the device.  A label outside [0, K) makes that row's loss, and so the loss, NaN; nothing is read or
 * written through it.  All five outputs are what the backward needs saved. */
int xvec_train_tail_forward(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                            const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K,
                            const int64_t* labels, float* pooled, float* a6, float* a7, float* logits, float* loss,
                            void* workspace, size_t workspace_bytes, xvec_stream stream);

/* dloss [1] is a DEVICE scalar (the incoming gradient of the loss).
 *   dlogits = dloss (softmax(logits) - onehot(labels)) / B
 *   dWo = dlogits^T a7, dbo = column sums of dlogits;   dz7 = [a7 > 0] dlogits Wo
 *   dW7 = dz7^T a6,     db7 = column sums of dz7;       dz6 = [a6 > 0] dz7 W7
 *   dW6 = dz6^T pooled, db6 = column sums of dz6;       (dmean, dstd) = dz6 W6
 *   dy5[b, t, c] = dmean[b, c] / Tp + dstd[b, c] (y5[b, t, c] - mean[b, c]) / ((Tp - 1) std[b, c]),
 *                  the second term 0 where std == 0 (what torch's std backward does).  Written once.  dy5 may be NULL. */
int xvec_train_tail_backward(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                             const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled,
                             const float* a6, const float* a7, const float* logits, float* dy5, float* dW6, float* db6,
                             float* dW7, float* db7, float* dWo, float* dbo, void* workspace, size_t workspace_bytes,
                             xvec_stream stream);

/* The two tail calls over a ragged batch: `lengths_dev` holds the valid frames of y5 [B, Tp, C] per utterance, 2 <= v5[b] <= Tp.
 * In the formulas above Tp becomes v5[b], the sums run over the first v5[b] frames, and dy5 is 0 on the others. */
int xvec_train_tail_forward_ragged(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                                   const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K,
                                   const int64_t* labels, float* pooled, float* a6, float* a7, float* logits, float* loss,
                                   void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev);
int xvec_train_tail_backward_ragged(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                                    const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled,
                                    const float* a6, const float* a7, const float* logits, float* dy5, float* dW6, float* db6,
                                    float* dW7, float* db7, float* dWo, float* dbo, void* workspace, size_t workspace_bytes,
                                    xvec_stream stream, const int32_t* lengths_dev);

/* torch.optim.Adam with its defaults (no amsgrad, no weight decay, not maximize) on n_tensors tensors, step count t >= 1:
 *   m = beta1 m + (1 - beta1) g,   v = beta2 v + (1 - beta2) g^2,
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * The four tables are HOST arrays of n_tensors DEVICE pointers, lengths_host their element counts.  The two bias
 * corrections are computed in double on the host; one launch updates up to 32 tensors (the table travels in the kernel's
 * argument block), more are chunked.  Any length and any 4-byte aligned base work. */
int xvec_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                   float* const* exp_avg_sq_host, const int64_t* lengths_host, int32_t n_tensors, double lr, double beta1,
                   double beta2, double eps, int64_t t, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_TRAIN_H */
