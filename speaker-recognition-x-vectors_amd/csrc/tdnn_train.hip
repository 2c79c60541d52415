// One TDNN layer in training mode, forward and backward, fp32 (reference tdnn_layer.py:26-41 under model.train()): the calls
// over full-length utterances.  C ABI: include/xvec_train.h.  Kernels and host code: tdnn_train_impl.h, here in the unmasked
// instantiation; the length-masked calls are tdnn_train_ragged.hip.  This file also owns the training calls' error channel.
#include "tdnn_train_impl.h"

namespace xvec {
namespace {
thread_local ErrorChannel g_terr;
}  // namespace

ErrorChannel& train_error_channel() { return g_terr; }

}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_train_last_error(void) { return g_terr.c_str(); }

size_t xvec_tdnn_train_workspace_bytes(int32_t B, int32_t T, int32_t Cin, int32_t Cout, const int32_t* context_host,
                                       int32_t n_ctx) {
    Shape s;
    if (make_shape(B, T, Cin, Cout, context_host, n_ctx, s)) return 0;
    return make_plan(nullptr, s).total;
}

int xvec_tdnn_train_forward(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                            int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                            const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                            void* workspace, size_t workspace_bytes, xvec_stream stream) {
    return train_forward<false>(x, B, T, Cin, W, bias, Cout, context_host, n_ctx, gamma, beta, eps, z, batch_mean, batch_var, y,
                                nullptr, workspace, workspace_bytes, stream);
}

int xvec_tdnn_train_backward(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                             const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                             const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                             float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                             size_t workspace_bytes, xvec_stream stream) {
    return train_backward<false>(dy, x, z, B, T, Cin, W, Cout, context_host, n_ctx, gamma, batch_mean, batch_var, eps, dx, dW,
                                 dbias, dgamma, dbeta, nullptr, workspace, workspace_bytes, stream);
}

}  // extern "C"
