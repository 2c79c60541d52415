// fp32 one-tap layers (4 and 5) as bf16_split3: the 128x128 kernel family's body (tdnn_layer_impl.h) with template flag S3 --
// activations split into hi | mid | lo bf16 planes on their way to LDS, weights pre-split by pack.hip, six bf16 products per
// 16-wide k-step on v_mfma_f32_32x32x16_bf16.  Its own translation unit: the store (layer 4) and pooling (layer 5)
// instantiations.
#include "tdnn_layer_impl.h"

namespace xvec {

// bf16_split3 instantiations of the fp32 one-tap layers: the store (layer 4) and pooling (layer 5) variants
template <bool POOL, bool STORE>
__global__ __launch_bounds__(256, 2) void tdnn_split3_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tdnn_body<false, POOL, STORE, false, false, false, true>(a, smem);
}

hipError_t launch_tdnn_split3(const TdnnArgs& a, bool pool, hipStream_t s) {
    static LdsOptIn opt_store, opt_pool;     // per variant and device
    if (a.n_taps != 1) return hipErrorInvalidValue;
    return pool ? launch_kernel(tdnn_split3_kernel<true, false>, a, s, opt_pool)
                : launch_kernel(tdnn_split3_kernel<false, true>, a, s, opt_store);
}

}  // namespace xvec
