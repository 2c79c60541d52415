// The dropout mask of the training layers (include/xvec_train.h, "Dropout"): ONE stateless function of (seed, stream, row,
// channel, p), shared by the forward product's epilogue (csrc/tdnn_train_dropout.hip) and the host (xvec_dropout_keep_host).
// Host-compilable (no HIP header, like mfcc_tables.h): __host__ __device__ under hipcc, plain inline C++ otherwise.
//
// The generator is Philox4x32-10 (philox.h; shared with the bootstrap, boot_plan.h): a 128-bit counter and
// a 64-bit key give four 32-bit words, with no state between calls.  Element (n, c) -- row n of the padded [B * T'] layout,
// output channel c -- is decided by word n & 3 of
//     philox(counter = (c, n >> 2, stream_lo, stream_hi), key = (seed_lo, seed_hi)):
// dropped iff word < thr, thr = floor(p * 2^32).  Four consecutive rows of one channel share a call: in the C/D layout of the
// 32 x 32 MFMA a lane holds the rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of one column and tile origins are multiples of 128,
// so the four accumulators r & 3 of a lane are the four words of one call.
#pragma once
#include <cstdint>

#include "philox.h"

#if defined(__HIPCC__)
#define XVEC_HD __host__ __device__ __forceinline__
#else
#define XVEC_HD inline
#endif

namespace xvec {
namespace dropout {

using philox::Words;
using philox::philox4x32_10;

// the four words of rows 4 * quad .. 4 * quad + 3 of channel c
XVEC_HD Words row_quad_words(uint32_t c, uint32_t quad, uint64_t seed, uint64_t stream) {
    return philox4x32_10(c, quad, (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 0 <= p < 1 (NaN fails both comparisons' conjunction)
XVEC_HD bool valid_p(float p) { return p >= 0.0f && p < 1.0f; }

// an element is dropped iff its word < threshold(p)
XVEC_HD uint32_t threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

// kept elements are multiplied by this, one fp32 multiply
XVEC_HD float keep_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

XVEC_HD bool keep(uint32_t n, uint32_t c, uint32_t thr, uint64_t seed, uint64_t stream) {
    return row_quad_words(c, n >> 2, seed, stream).w[n & 3] >= thr;
}

}  // namespace dropout
}  // namespace xvec

#undef XVEC_HD
