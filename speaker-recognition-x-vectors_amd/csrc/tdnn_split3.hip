// fp32 one-tap layers (4 and 5) as bf16_split3: the 128x128 kernel family's body (tdnn_layer_impl.h) with template flag S3 --
// activations split into hi | mid | lo bf16 planes on their way to LDS, weights pre-split by pack.hip, six bf16 products per
// 16-wide k-step on v_mfma_f32_32x32x16_bf16.  Its own translation unit: the store (layer 4) and pooling (layer 5)
// instantiations.
#include "tdnn_layer_impl.h"

namespace xvec {

// bf16_split3 instantiations of the fp32 one-tap layers: the store (layer 4) and pooling (layer 5) variants
template <bool POOL, bool STORE>
__global__ __launch_bounds__(256, 3) void tdnn_split3_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tdnn_body<false, POOL, STORE, false, false, false, true>(a, smem);
}

static LdsOptIn opt_store, opt_pool;     // per variant and device

hipError_t launch_tdnn_split3(const TdnnArgs& a, bool pool, hipStream_t s) {
    if (a.n_taps != 1) return hipErrorInvalidValue;
    return pool ? launch_kernel(tdnn_split3_kernel<true, false>, a, s, opt_pool, kS3LdsBytes)
                : launch_kernel(tdnn_split3_kernel<false, true>, a, s, opt_store, kS3LdsBytes);
}

hipError_t tdnn_split3_max_blocks_per_cu(int* blocks) {
    const void* kern[2] = {reinterpret_cast<const void*>(tdnn_split3_kernel<false, true>),
                           reinterpret_cast<const void*>(tdnn_split3_kernel<true, false>)};
    LdsOptIn* opt[2] = {&opt_store, &opt_pool};
    int least = 0;
    for (int v = 0; v < 2; ++v) {
        int n = 0;
        if (hipError_t e = opt[v]->ensure(kern[v], kS3LdsBytes); e != hipSuccess) return e;
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern[v], 256, kS3LdsBytes); e != hipSuccess) return e;
        least = v == 0 ? n : (n < least ? n : least);
    }
    *blocks = least;
    return hipSuccess;
}

}  // namespace xvec
