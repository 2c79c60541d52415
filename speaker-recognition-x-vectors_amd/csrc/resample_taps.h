// The tap plan of sinc resampling (csrc/resample.hip, include/xvec_resample.h): what one ratio turns into (inc, scale, step), how
// many outputs a row of n samples gives, and for output t of a row which input sample is its centre, where in the filter table
// each wing starts, the interpolation weight between two table entries, and how many taps each wing has.  Everything is fp64,
// one IEEE operation per line of the algorithm in the header, never contracted: the plan must be bit for bit what numpy computes
// for the same row.  Host-compilable (no HIP header, like snorm_keys.h and dropout_mask.h): __host__ __device__ under hipcc, plain
// inline C++ otherwise, so that tests/test_resample.py can check it on the CPU (tests/abi/resample_taps_dump.cpp, built with
// -ffp-contract=off where the compiler does not know the pragma below).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define XVEC_RESAMPLE_FN __host__ __device__ __forceinline__
#else
#define XVEC_RESAMPLE_FN inline
#endif

namespace xvec {
namespace resample_taps {

// What a ratio = sr_new / sr_orig becomes.  Downsampling (ratio < 1) scales the table by the ratio and walks it in steps of
// int(ratio * P) entries -- TRUNCATED, as resampy 0.3.0 does: 512 / 3 becomes 170, which widens the filter a little and leaves
// an error of 2.7e-3 on a 48 kHz -> 16 kHz sine.  Kept, because the bits of the package are the contract.
struct RatioPlan {
    double ratio;      // sr_new / sr_orig
    double inc;        // 1.0 / ratio: input samples per output
    double scale;      // min(1.0, ratio)
    int32_t step;      // int(scale * P): table entries per input sample
    int32_t scaled;    // ratio < 1: the table is multiplied by the ratio
};

XVEC_RESAMPLE_FN bool ratio_ok(double ratio) { return ratio > 0.0 && ratio <= 1.7976931348623157e308; }      // false for NaN

// P = 2 ** precision table entries per zero crossing.  step < 1 (ratio < 1 / P) is for the caller to refuse.
XVEC_RESAMPLE_FN RatioPlan plan_ratio(double ratio, int32_t P) {
    RatioPlan r;
    r.ratio = ratio;
    r.inc = 1.0 / ratio;
    r.scale = ratio < 1.0 ? ratio : 1.0;
    const double s = r.scale * (double)P;
    r.step = (int32_t)s;
    r.scaled = ratio < 1.0 ? 1 : 0;
    return r;
}

// n_out = int(n * ratio): outputs of a row of n samples (0 is a row without outputs; the package raises there).  Saturates at
// 2^62 instead of overflowing.
XVEC_RESAMPLE_FN int64_t out_len(int64_t n, double ratio) {
    const double v = (double)n * ratio;
    return v >= 4611686018427387904.0 ? (int64_t)1 << 62 : (int64_t)v;
}

// The largest number of taps a wing can have: the walk from table offset 0.
XVEC_RESAMPLE_FN int64_t max_taps(int64_t nwin, int32_t step) { return nwin / step; }

// Input samples a tile of `tile` consecutive outputs can touch, at most: the centres span floor((tile - 1) * inc) + 1 samples,
// each wing adds max_taps.  What decides whether a row's tiles are staged in LDS.
XVEC_RESAMPLE_FN int64_t tile_span(const RatioPlan& r, int64_t nwin, int32_t tile) {
    const double c = (double)(tile - 1) * r.inc;
    if (!(c < 4611686018427387904.0)) return (int64_t)1 << 62;
    return (int64_t)c + 1 + 2 * max_taps(nwin, r.step);
}

struct TapPlan {
    int64_t n0;        // centre: the left wing reads x[n0 - i], the right wing x[n0 + 1 + k]
    int32_t off_l;     // table entry of the left wing's tap 0; tap i is entry off_l + i * step
    int32_t off_r;
    double eta_l;      // weight of tap i: win_s[j] + eta * (win_s[j + 1] - win_s[j])
    double eta_r;
    int64_t i_min;     // 0 unless n0 >= n (t * inc rounded up to the row's end at an extreme ratio): taps that would leave the row
    int64_t i_max;     // left wing: i in [i_min, i_max), ascending
    int64_t k_max;     // right wing: k in [0, k_max), ascending, after the left wing
};

// Output t of a row of n samples.
XVEC_RESAMPLE_FN TapPlan plan_output(int64_t t, const RatioPlan& r, int32_t P, int64_t nwin, int64_t n) {
    TapPlan p;
    const double time = (double)t * r.inc;
    p.n0 = (int64_t)time;
    double frac = r.scale * (time - (double)p.n0);
    double idx = frac * (double)P;
    p.off_l = (int32_t)idx;
    p.eta_l = idx - (double)p.off_l;
    const int64_t wl = (nwin - p.off_l) / r.step;
    p.i_max = p.n0 + 1 < wl ? p.n0 + 1 : wl;
    p.i_min = p.n0 >= n ? p.n0 - (n - 1) : 0;
    if (p.i_min > p.i_max) p.i_min = p.i_max;
    frac = r.scale - frac;
    idx = frac * (double)P;
    p.off_r = (int32_t)idx;
    p.eta_r = idx - (double)p.off_r;
    const int64_t wr = (nwin - p.off_r) / r.step;
    const int64_t room = n - p.n0 - 1;
    p.k_max = room < wr ? room : wr;
    if (p.k_max < 0) p.k_max = 0;
    return p;
}

}  // namespace resample_taps
}  // namespace xvec
