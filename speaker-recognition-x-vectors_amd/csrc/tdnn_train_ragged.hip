// One TDNN layer in training mode over a RAGGED batch on the padded layout x [B, T, Cin]: per-utterance valid-frame counts on
// the device, everything that depends on them computed there (no read-back, no synchronisation).  C ABI: include/xvec_train.h.
// Kernels and host code: tdnn_train_impl.h, here in the length-masked instantiation.
#include "tdnn_train_impl.h"

using namespace xvec;

extern "C" {

int xvec_tdnn_train_forward_ragged(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                                   int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                                   const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                                   void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev) {
    return train_forward<true>(x, B, T, Cin, W, bias, Cout, context_host, n_ctx, gamma, beta, eps, z, batch_mean, batch_var, y,
                               lengths_dev, workspace, workspace_bytes, stream);
}

int xvec_tdnn_train_backward_ragged(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                                    const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                                    const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                                    float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                    size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev) {
    return train_backward<true>(dy, x, z, B, T, Cin, W, Cout, context_host, n_ctx, gamma, batch_mean, batch_var, eps, dx, dW,
                                dbias, dgamma, dbeta, lengths_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
