// The tail of a training step over a RAGGED batch on the padded layout y5 [B, Tp, C]: the pooling and its backward run over each
// utterance's valid frames (device lengths, no read-back), everything after the pooling is per utterance and is train_tail.hip's
// own code.  C ABI: include/xvec_train.h.  The kernels here are the length-masked instantiation of train_tail_pool.h.
#include "train_tail_pool.h"

using namespace xvec;

extern "C" {

int xvec_train_tail_forward_ragged(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                                   const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K,
                                   const int64_t* labels, float* pooled, float* a6, float* a7, float* logits, float* loss,
                                   void* workspace, size_t workspace_bytes, xvec_stream stream, const int32_t* lengths_dev) {
    if (!lengths_dev) return train_error_channel().fail(XVEC_ERR_ARG, "null pointer: lengths_dev");
    return train_tail_forward(y5, B, Tp, C, W6, b6, H, W7, b7, Wo, bo, K, labels, pooled, a6, a7, logits, loss, workspace,
                              workspace_bytes, stream, launch_tail_pool<true>, lengths_dev);
}

int xvec_train_tail_backward_ragged(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                                    const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled,
                                    const float* a6, const float* a7, const float* logits, float* dy5, float* dW6, float* db6,
                                    float* dW7, float* db7, float* dWo, float* dbo, void* workspace, size_t workspace_bytes,
                                    xvec_stream stream, const int32_t* lengths_dev) {
    if (!lengths_dev) return train_error_channel().fail(XVEC_ERR_ARG, "null pointer: lengths_dev");
    return train_tail_backward(dloss, y5, B, Tp, C, W6, H, W7, Wo, K, labels, pooled, a6, a7, logits, dy5, dW6, db6, dW7, db7, dWo,
                               dbo, workspace, workspace_bytes, stream, launch_tail_pool_bwd<true>, lengths_dev);
}

}  // extern "C"
