// One TDNN layer in training mode with dropout after the ReLU (reference tdnn_layer.py:26-41: Linear, ReLU, Dropout,
// BatchNorm), over full-length or ragged batches.  C ABI: include/xvec_train.h.  Kernels and host code: tdnn_train_impl.h, here
// in the dropout instantiation: the forward product's epilogue draws the mask from dropout_mask.h (nothing is stored), the dz
// kernel carries the scale of the kept elements; every other kernel of the two calls is the one the calls without dropout
// launch.  xvec_dropout_keep_host evaluates the same header on the CPU.
#include "tdnn_train_impl.h"

using namespace xvec;

extern "C" {

int xvec_tdnn_train_forward_dropout(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias,
                                    int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma,
                                    const float* beta, float eps, float* z, float* batch_mean, float* batch_var, float* y,
                                    void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev,
                                    float p, uint64_t seed, uint64_t dropout_stream) {
    Dropout<true> D;
    if (int rc = make_dropout(p, seed, dropout_stream, D)) return rc;
    if (lengths_dev)
        return train_forward<true, true>(x, B, T, Cin, W, bias, Cout, context_host, n_ctx, gamma, beta, eps, z, batch_mean,
                                         batch_var, y, lengths_dev, workspace, workspace_bytes, stream, D);
    return train_forward<false, true>(x, B, T, Cin, W, bias, Cout, context_host, n_ctx, gamma, beta, eps, z, batch_mean, batch_var,
                                      y, nullptr, workspace, workspace_bytes, stream, D);
}

int xvec_tdnn_train_backward_dropout(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin,
                                     const float* W, int32_t Cout, const int32_t* context_host, int32_t n_ctx,
                                     const float* gamma, const float* batch_mean, const float* batch_var, float eps, float* dx,
                                     float* dW, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                     size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev, float p) {
    Dropout<true> D;
    if (int rc = make_dropout(p, 0, 0, D)) return rc;
    if (lengths_dev)
        return train_backward<true, true>(dy, x, z, B, T, Cin, W, Cout, context_host, n_ctx, gamma, batch_mean, batch_var, eps, dx,
                                          dW, dbias, dgamma, dbeta, lengths_dev, workspace, workspace_bytes, stream, D);
    return train_backward<false, true>(dy, x, z, B, T, Cin, W, Cout, context_host, n_ctx, gamma, batch_mean, batch_var, eps, dx, dW,
                                       dbias, dgamma, dbeta, nullptr, workspace, workspace_bytes, stream, D);
}

int xvec_dropout_keep_host(uint8_t* keep_host, int64_t N, int32_t Cout, float p, uint64_t seed, uint64_t dropout_stream) {
    if (!keep_host) return terr().fail(XVEC_ERR_ARG, "null pointer: keep_host");
    if (N < 1 || Cout < 1) return terr().fail(XVEC_ERR_ARG, "N = %lld and Cout = %d must be >= 1", (long long)N, Cout);
    if (N > 0x7fffffff) return terr().fail(XVEC_ERR_TOO_LARGE, "N = %lld rows: row indices are int32", (long long)N);
    Dropout<true> D;
    if (int rc = make_dropout(p, seed, dropout_stream, D)) return rc;
    for (int64_t quad = 0; quad * 4 < N; ++quad)
        for (int32_t c = 0; c < Cout; ++c) {
            const dropout::Words w = dropout::row_quad_words((uint32_t)c, (uint32_t)quad, seed, dropout_stream);
            for (int r = 0; r < 4 && quad * 4 + r < N; ++r) keep_host[(quad * 4 + r) * Cout + c] = w.w[r] >= D.thr;
        }
    return XVEC_OK;
}

}  // extern "C"
