/* xvec_train.h -- C ABI of the training-mode TDNN layer in libxvec_hip.so.
 *
 * One frame-level layer of the reference (tdnn_layer.py:26-41) as its training loop runs it (main.py:97-101 under
 * model.train()): context gather, Linear, ReLU and BatchNorm1d on the BATCH statistics, forward and backward.  The five
 * frame-level layers are 99.7 % of a training step's arithmetic; pooling, the segment layers, the loss and the optimizer
 * stay on torch ops for now (xvector_amd.train).
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

#ifdef __cplusplus
}
#endif
#endif /* XVEC_TRAIN_H */
