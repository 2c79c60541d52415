// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): a 128-bit counter and a 64-bit key give
// four 32-bit words, with no state between calls.  ONE generator for the dropout masks (dropout_mask.h) and the bootstrap
// weights (boot_plan.h).  Host-compilable (no HIP header): __host__ __device__ under hipcc, plain inline C++ otherwise.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XVEC_PHILOX_HD __host__ __device__ __forceinline__
#else
#define XVEC_PHILOX_HD inline
#endif

namespace xvec {
namespace philox {

struct Words {
    uint32_t w[4];
};

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;     // round multipliers
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;     // key increments (golden ratio, sqrt(3) - 1)

// ten rounds; the key is bumped between rounds (nine times)
XVEC_PHILOX_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)kMul0 * c0, p1 = (uint64_t)kMul1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kKey0;
        k1 += kKey1;
    }
    return Words{{c0, c1, c2, c3}};
}

}  // namespace philox
}  // namespace xvec

#undef XVEC_PHILOX_HD
