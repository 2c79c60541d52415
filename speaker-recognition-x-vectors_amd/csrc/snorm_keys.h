// The order-preserving key of an fp64 score and the digit walk of the radix select over it (csrc/snorm.hip): which 64-bit key a
// cell gets, which cells are NaN, how a key goes back to its value, which digit a pass looks at and which digit of a pass's
// histogram holds the k-th largest key.  Host-compilable (no HIP header, like score_tiles.h and dropout_mask.h):
// __device__ __forceinline__ under hipcc, plain inline C++ otherwise, so that tests/test_snorm.py can check the map and the walk
// on the CPU (tests/abi/snorm_keys_dump.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XVEC_SNORM_FN __host__ __device__ __forceinline__
#else
#define XVEC_SNORM_FN inline
#endif

namespace xvec {
namespace snorm_keys {

constexpr int kDigitBits = 8;                        // one pass of the select looks at 8 bits of the key
constexpr int kRadix = 1 << kDigitBits;              // bins of a pass's histogram
constexpr int kPasses = 64 / kDigitBits;             // most significant digit first
constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr uint64_t kExpMask = 0x7ff0000000000000ull;
// The key of a cell that takes no part (NaN, skipped column).  No value maps to it: the smallest key of a value is that of
// -inf, 0x000fffffffffffff.
constexpr uint64_t kKeyVoid = 0;

XVEC_SNORM_FN uint64_t bits_of(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

XVEC_SNORM_FN double value_of_bits(uint64_t u) {
    double x;
    memcpy(&x, &u, sizeof(x));
    return x;
}

// NaN: exponent all ones and a mantissa that is not zero (quiet or signalling, either sign)
XVEC_SNORM_FN bool is_nan_bits(uint64_t u) { return (u & ~kSign) > kExpMask; }

// key(a) < key(b) iff a < b for all a, b that are not NaN; -0.0 and +0.0 share 0x8000000000000000; +-inf are ordinary values.
// Not to be called on a NaN (is_nan_bits first).
XVEC_SNORM_FN uint64_t key_of_bits(uint64_t u) {
    if ((u << 1) == 0) u = 0;                         // -0.0 -> +0.0
    return (u & kSign) ? ~u : (u | kSign);
}

// The inverse: the bits of the value a key stands for (+0.0 for the key the two zeros share).
XVEC_SNORM_FN uint64_t bits_of_key(uint64_t k) { return (k & kSign) ? (k ^ kSign) : ~k; }

XVEC_SNORM_FN uint64_t key_of(double x) { return key_of_bits(bits_of(x)); }
XVEC_SNORM_FN double value_of_key(uint64_t k) { return value_of_bits(bits_of_key(k)); }

// The key a cell enters the select with: kKeyVoid when it takes no part.
XVEC_SNORM_FN uint64_t cell_key(double x, bool skipped) {
    const uint64_t u = bits_of(x);
    return (skipped || is_nan_bits(u)) ? kKeyVoid : key_of_bits(u);
}

// Pass p (0 = first) looks at the p-th most significant digit.
XVEC_SNORM_FN int pass_shift(int pass) { return 64 - kDigitBits * (pass + 1); }
XVEC_SNORM_FN uint32_t digit_of(uint64_t key, int pass) { return (uint32_t)(key >> pass_shift(pass)) & (kRadix - 1); }

// A key takes part in pass p iff its digits of the passes before p are the ones chosen so far (`prefix`: those digits, most
// significant first, in the low bits).
XVEC_SNORM_FN bool in_prefix(uint64_t key, uint64_t prefix, int pass) {
    return pass == 0 || (key >> (pass_shift(pass) + kDigitBits)) == prefix;
}

// Digit d of a pass holds the k-th largest (k >= 1) of the keys taking part iff `above` of them have a larger digit and `count`
// have digit d with above < k <= above + count.  Exactly one digit does when 1 <= k <= the keys taking part; the walk goes on
// inside it for the (k - above)-th largest.
XVEC_SNORM_FN bool digit_holds_kth(uint32_t above, uint32_t count, uint32_t k) { return above < k && k <= above + count; }

// The whole walk on the host, one key at a time: the k-th largest key (1 <= k <= the keys that are not kKeyVoid) and, in
// *n_above, how many keys are larger.  What the kernel computes with a block per row; the CPU test compares it with a sort.
inline uint64_t select_kth_host(const uint64_t* keys, uint32_t n, uint32_t k, uint32_t* n_above) {
    uint64_t prefix = 0;
    uint32_t above_total = 0;
    for (int pass = 0; pass < kPasses; ++pass) {
        uint32_t hist[kRadix] = {};
        for (uint32_t i = 0; i < n; ++i)
            if (keys[i] != kKeyVoid && in_prefix(keys[i], prefix, pass)) ++hist[digit_of(keys[i], pass)];
        uint32_t above = 0;
        for (int d = kRadix - 1; d >= 0; --d) {
            if (digit_holds_kth(above, hist[d], k)) {
                prefix = (prefix << kDigitBits) | (uint32_t)d;
                k -= above;
                above_total += above;
                break;
            }
            above += hist[d];
        }
    }
    if (n_above) *n_above = above_total;
    return prefix;
}

}  // namespace snorm_keys
}  // namespace xvec
