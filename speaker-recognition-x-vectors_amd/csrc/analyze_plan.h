// The host side of score analysis (csrc/analyze.hip, include/xvec_analyze.h): the argument checks with one text per refusal,
// the persistent grid and the depth of its summation tree, the workspace layouts of both families, the bin map of the
// histogram (the kernels call it as it stands here), the rule for the LDS copies of the histogram, and the digit and candidate
// plan of the select.  Host-compilable (no HIP header), so that tests/test_analyze.py can ask it on the CPU
// (tests/abi/analyze_plan_dump.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_analyze.h"
#include "plan_support.h"
#include "snorm_keys.h"
#include "trial_plan.h"

#if defined(__HIPCC__)
#define XVEC_ANALYZE_HD __host__ __device__ __forceinline__
#else
#define XVEC_ANALYZE_HD inline
#endif

namespace xvec {
namespace analyze_plan {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;
constexpr int kTile = XVEC_ANALYZE_TILE;               // trials a block reads per step
constexpr int kMaxBlocks = XVEC_ANALYZE_MAX_BLOCKS;    // the persistent grid: a constant, so the summation tree is the same on every device
constexpr int kMaxBins = XVEC_ANALYZE_MAX_BINS;
constexpr int kMaxK = XVEC_ANALYZE_MAX_K;
constexpr int kMaxCand = XVEC_ANALYZE_MAX_CAND;
constexpr int kDefaultCand = 16384;
constexpr int kHistWords = 8192 + 64;                  // uint32 words of LDS the histogram copies share
constexpr int kMaxCopies = 32;                         // one copy per LDS bank at the most
constexpr int kRadix = snorm_keys::kRadix;
constexpr int kPasses = snorm_keys::kPasses;
constexpr int kPart1Bytes = 112;                       // a block's partial of pass 1 (analyze.hip: Part1)
constexpr int kPart2Bytes = 16;                        // and of pass 2: M2 of the two classes
constexpr int kStateBytes = 256;                       // the select's state (analyze.hip: SelState)
constexpr int kRecordBytes = 24;                       // xvec_analyze_record
constexpr int64_t kMaxFirst = (int64_t)1 << 52;        // |first| up to here is exact as a double, and so is first + n_bins
static_assert(kTile == kThreads * kItems, "include/xvec_analyze.h: XVEC_ANALYZE_TILE");
static_assert(kMaxBlocks % kThreads == 0, "the merge walks the blocks in strides of a block");

using trial_plan::count_ok;

// ---------------------------------------------------------------- the persistent grid

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
inline int64_t blocks_of(int64_t n) { const int64_t t = tiles_of(n); return t < kMaxBlocks ? t : kMaxBlocks; }
// block b of G walks the tiles [first_tile(b), first_tile(b + 1))
XVEC_ANALYZE_HD int64_t first_tile(int64_t b, int64_t tiles, int64_t G) { return b * tiles / G; }
inline int64_t most_tiles(int64_t n) { const int64_t t = tiles_of(n), g = blocks_of(n); return (t + g - 1) / g; }
// additions on the longest path from a term to the sum: the thread's running sum, butterfly, waves; then the same over the blocks
inline int64_t sum_depth(int64_t n) {
    return most_tiles(n) * kItems + 6 + (kWaves - 1) + (blocks_of(n) + kThreads - 1) / kThreads + 6 + (kWaves - 1);
}
constexpr int64_t kSecondTileFrom = (int64_t)kMaxBlocks * kTile + 1;

// ---------------------------------------------------------------- the bin map

// slot of score s (not NaN) among n_bins + 2: 0 underflow, b + 1 bin b, n_bins + 1 overflow.  The comparison is made on the
// rounded quotient as a double; only a value inside [first, first + n_bins - 1] is converted.
XVEC_ANALYZE_HD int32_t slot_of(double s, double width, int64_t first, int32_t n_bins, int32_t rounding) {
    const double q = s / width;
    const double r = rounding == XVEC_ANALYZE_RINT ? rint(q) : floor(q);
    const double lo = (double)first, hi = (double)(first + n_bins - 1);
    if (r < lo) return 0;
    if (r > hi) return n_bins + 1;
    return (int32_t)((int64_t)r - first) + 1;
}

// ---------------------------------------------------------------- the LDS copies of the histogram

inline int32_t slots_of(int32_t n_bins) { return 2 * (n_bins + 2); }
constexpr int32_t copy_stride(int32_t slots) { return slots + 1; }        // odd: the copies of a slot lie in different banks
// the most private copies a block keeps: the largest power of two of strides within kHistWords, at most kMaxCopies; 1 for large n_bins
inline int32_t max_copies(int32_t n_bins) {
    if (n_bins < 1 || n_bins > kMaxBins) return 0;
    const int32_t fit = kHistWords / copy_stride(slots_of(n_bins));
    int32_t c = 1;
    while (c * 2 <= fit && c * 2 <= kMaxCopies) c *= 2;
    return c;
}
inline int32_t copies_of(int32_t n_bins, int32_t asked) { return asked ? asked : max_copies(n_bins); }
static_assert(copy_stride(2 * (kMaxBins + 2)) <= kHistWords, "XVEC_ANALYZE_MAX_BINS: one copy must fit");

// ---------------------------------------------------------------- the select

inline int32_t cand_cap_of(int32_t k, int32_t asked) { return asked ? asked : (k > kDefaultCand ? k : kDefaultCand); }
// a pass that chose p digits compares key >> shift_after(p) with the prefix
XVEC_ANALYZE_HD int shift_after(int p) { return 64 - snorm_keys::kDigitBits * p; }

// ---------------------------------------------------------------- workspaces

struct SummaryLayout {
    size_t part1, part2, total;      // [blocks] partials of the two passes; total 0: refused
    int64_t tiles, blocks;
};

inline SummaryLayout summary_layout(int64_t n, int32_t n_bins) {
    if (!count_ok(n) || n_bins < 0 || n_bins > kMaxBins) return SummaryLayout{};
    SummaryLayout l{};
    l.tiles = tiles_of(n);
    l.blocks = blocks_of(n);
    Carver c;
    l.part1 = c.take_bytes((size_t)l.blocks * kPart1Bytes);
    l.part2 = c.take_bytes((size_t)l.blocks * kPart2Bytes);
    l.total = c.total();
    return l;
}

struct HardestLayout {
    size_t hist;                     // uint32 [kPasses][2][kRadix], cleared
    size_t state;                    // SelState, cleared with it (it follows hist)
    size_t counts, offsets;          // uint32 [4][kMaxBlocks]: greater / equal of class 0, of class 1, per block; their scan
    size_t cand[2];                  // xvec_analyze_record [cap] per class
    size_t total;
    int64_t tiles, blocks;
    int32_t cap;
};

inline bool select_ok(int32_t k, int32_t cand_cap) {
    return k >= 1 && k <= kMaxK && (cand_cap == 0 || (cand_cap >= k && cand_cap <= kMaxCand));
}

inline HardestLayout hardest_layout(int64_t n, int32_t k, int32_t cand_cap) {
    if (!count_ok(n) || !select_ok(k, cand_cap)) return HardestLayout{};
    HardestLayout l{};
    l.tiles = tiles_of(n);
    l.blocks = blocks_of(n);
    l.cap = cand_cap_of(k, cand_cap);
    Carver c;
    l.hist = c.take_bytes((size_t)kPasses * 2 * kRadix * 4);
    l.state = c.take_bytes(kStateBytes);
    l.counts = c.take_bytes((size_t)4 * kMaxBlocks * 4);
    l.offsets = c.take_bytes((size_t)4 * kMaxBlocks * 4);
    for (int i = 0; i < 2; ++i) l.cand[i] = c.take_bytes((size_t)l.cap * kRecordBytes);
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_bins(const xvec_analyze_bins* b, const void* counts, Refusal& why) {
    if (!b) return 0;
    if (b->n_bins < 1 || b->n_bins > kMaxBins) return why.refuse("n_bins = %d must lie in 1 .. %d", b->n_bins, kMaxBins);
    if (!(b->width > 0.0) || !(b->width <= 1.7976931348623157e308))
        return why.refuse("width = %g must be positive and finite", b->width);
    if (b->first < -kMaxFirst || b->first > kMaxFirst)
        return why.refuse("first = %lld must lie in -2^52 .. 2^52", (long long)b->first);
    if (b->rounding != XVEC_ANALYZE_FLOOR && b->rounding != XVEC_ANALYZE_RINT)
        return why.refuse("rounding = %d must be 0 (floor) or 1 (rint)", b->rounding);
    const int32_t c = b->hist_copies;
    if (c < 0 || (c & (c - 1)) != 0 || c > max_copies(b->n_bins))
        return why.refuse("hist_copies = %d must be 0 or a power of two up to %d for %d bins", c, max_copies(b->n_bins), b->n_bins);
    if (b->reserved != 0) return why.refuse("reserved = %d must be 0", b->reserved);
    if (!counts) return why.refuse("null pointer: counts");
    return 0;
}

inline int check_stats(const void* out, Refusal& why) {
    if (!out) return why.refuse("null pointer: out");
    return 0;
}

inline int check_select(const xvec_analyze_select* s, Refusal& why) {
    if (!s) return why.refuse("null pointer: select");
    if (s->k < 1 || s->k > kMaxK) return why.refuse("k = %d must lie in 1 .. %d", s->k, kMaxK);
    if (s->cand_cap != 0 && (s->cand_cap < s->k || s->cand_cap > kMaxCand))
        return why.refuse("cand_cap = %d must be 0 or lie in k = %d .. %d", s->cand_cap, s->k, kMaxCand);
    return 0;
}

inline int check_lists(const void* nontarget_out, const void* target_out, const void* counts, Refusal& why) {
    if (!nontarget_out || !target_out) return why.refuse("null pointer: nontarget_out / target_out");
    if (!counts) return why.refuse("null pointer: counts");
    return 0;
}

inline int check_plan_query(int64_t n, int32_t n_bins, const void* out, Refusal& why) {
    if (!count_ok(n)) return why.refuse("n_trials = %lld must lie in 1 .. 2^31 - 1", (long long)n);
    if (n_bins < 0 || n_bins > kMaxBins) return why.refuse("n_bins = %d must lie in 0 .. %d", n_bins, kMaxBins);
    if (!out) return why.refuse("null pointer: out");
    return 0;
}

}  // namespace analyze_plan
}  // namespace xvec

#undef XVEC_ANALYZE_HD
