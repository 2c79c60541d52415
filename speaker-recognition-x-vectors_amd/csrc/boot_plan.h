// The host side of the bootstrap (csrc/boot.hip, include/xvec_boot.h): the argument checks with one text per refusal, the
// workspace layout, the batching of the replicates, and the two maps word -> group and word -> Poisson weight, which the
// kernels call as they stand here.  Host-compilable (no HIP header), so that tests/test_bootstrap.py can ask it on the CPU
// (tests/abi/boot_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_boot.h"
#include "philox.h"
#include "plan_support.h"
#include "trial_plan.h"

#if defined(__HIPCC__)
#define XVEC_BOOT_HD __host__ __device__ __forceinline__
#else
#define XVEC_BOOT_HD inline
#endif

namespace xvec {
namespace boot_plan {

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;               // the sort's tile (trial_sort.h)
constexpr int kRadix = 256;
constexpr int kMaxGroups = XVEC_BOOT_MAX_GROUPS;
constexpr int kMaxBoot = XVEC_BOOT_MAX_BOOT;
constexpr uint32_t kMagic = XVEC_BOOT_MAGIC;
constexpr int kChunk = 8;                              // replicates a block walks over one load of its tile
constexpr int kMaxBatch = 256;                         // replicates per batch, at the most
constexpr int64_t kPartials = 1 << 20;                 // (replicate, tile) partials a batch may hold
constexpr int kCounters = 8;                           // uint64 each: see boot.hip
constexpr int kPartialBytes = 16 + 24 + 24 + 8;        // per (replicate, tile): two 64-bit sums, an EerCand, a DcfCand, its `below`
constexpr int64_t kOverflow = (int64_t)1 << 31;        // a replicate of this many weighted trials is not evaluated

using trial_plan::count_ok;

// ---------------------------------------------------------------- the two maps

// draw -> group: word j & 3 of philox(j >> 2, b, side, MAGIC) picks (word * G) >> 32
XVEC_BOOT_HD uint32_t pick_group(uint32_t word, uint32_t n_groups) { return (uint32_t)(((uint64_t)word * n_groups) >> 32); }

// T_i = floor(2^32 P[Poisson(1) <= i]); the table ends where it reaches 2^32 - 1
constexpr int kPoissonTerms = XVEC_BOOT_POISSON_TERMS;
#define XVEC_BOOT_POISSON_TABLE(X)                                                                                          \
    X(0x5e2d58d8u) X(0xbc5ab1b1u) X(0xeb715e1du) X(0xfb239797u) X(0xff1025f5u) X(0xffd90f3bu) X(0xfffa8b71u) X(0xffff540cu) \
    X(0xffffed1fu) X(0xfffffe21u) X(0xffffffd4u) X(0xfffffffcu) X(0xffffffffu)

// (host only: the table for the dump program)
inline uint32_t poisson_threshold(int i) {
#define XVEC_BOOT_ENTRY(T) T,
    const uint32_t t[] = {XVEC_BOOT_POISSON_TABLE(XVEC_BOOT_ENTRY)};
#undef XVEC_BOOT_ENTRY
    static_assert(sizeof(t) == kPoissonTerms * sizeof(uint32_t), "include/xvec_boot.h: XVEC_BOOT_POISSON_TERMS");
    return t[i];
}

// word -> Poisson(1) weight: the number of i with word >= T_i (thirteen compares on constants: no table in memory)
XVEC_BOOT_HD uint32_t poisson_weight(uint32_t word) {
    uint32_t w = 0;
#define XVEC_BOOT_STEP(T) w += word >= T;
    XVEC_BOOT_POISSON_TABLE(XVEC_BOOT_STEP)
#undef XVEC_BOOT_STEP
    return w;
}

XVEC_BOOT_HD philox::Words draw_words(uint32_t quad, uint32_t b, uint32_t side, uint64_t seed) {
    return philox::philox4x32_10(quad, b, side, kMagic, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// word i of a call, by selection: an index into the four would put them in memory
XVEC_BOOT_HD uint32_t word_of(const philox::Words& w, uint32_t i) {
    return i == 0 ? w.w[0] : i == 1 ? w.w[1] : i == 2 ? w.w[2] : w.w[3];
}

// the group that draw j of (seed, b, side) picks among n_groups
XVEC_BOOT_HD uint32_t drawn_group(uint64_t seed, uint32_t b, uint32_t side, uint32_t j, uint32_t n_groups) {
    return pick_group(word_of(draw_words(j >> 2, b, side, seed), j & 3), n_groups);
}

// the Poisson weight of original trial t in replicate b
XVEC_BOOT_HD uint32_t trial_poisson(uint64_t seed, uint32_t b, uint32_t t) {
    return poisson_weight(word_of(draw_words(t >> 2, b, 2u, seed), t & 3));
}

// ---------------------------------------------------------------- the packed payload of a sorted trial

// group mode: row group (14 bits), column group (14 bits), target bit (2 bits; 2 = left out)
XVEC_BOOT_HD uint32_t pack_groups(uint32_t gr, uint32_t gc, uint32_t bit) { return gr | (gc << 14) | (bit << 28); }
XVEC_BOOT_HD uint32_t packed_row(uint32_t p) { return p & 0x3fffu; }
XVEC_BOOT_HD uint32_t packed_col(uint32_t p) { return (p >> 14) & 0x3fffu; }
XVEC_BOOT_HD uint32_t packed_bit(uint32_t p) { return p >> 28; }
// Poisson mode: the trial's index (31 bits) and its target bit on top
XVEC_BOOT_HD uint32_t pack_index(uint32_t t, uint32_t bit) { return t | (bit << 31); }
XVEC_BOOT_HD uint32_t packed_index(uint32_t p) { return p & 0x7fffffffu; }
XVEC_BOOT_HD uint32_t packed_index_bit(uint32_t p) { return p >> 31; }

// ---------------------------------------------------------------- batching: functions of (n, n_boot)

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// Records 0 .. n_boot are processed `batch` at a time: a multiple of kChunk, as many as keep the partials of a batch within
// kPartials (tile, replicate) pairs, at most kMaxBatch, and no more than there are records.  0: refused.
inline int32_t batch_size(int64_t n, int64_t n_boot) {
    if (!count_ok(n) || n_boot < 1 || n_boot > kMaxBoot) return 0;
    int64_t b = kPartials / tiles_of(n) / kChunk * kChunk;
    if (b < kChunk) b = kChunk;
    if (b > kMaxBatch) b = kMaxBatch;
    const int64_t all = (n_boot + 1 + kChunk - 1) / kChunk * kChunk;
    return (int32_t)(b < all ? b : all);
}

inline int32_t batch_count(int64_t n, int64_t n_boot) {
    const int32_t b = batch_size(n, n_boot);
    return b ? (int32_t)((n_boot + 1 + b - 1) / b) : 0;
}

// ---------------------------------------------------------------- workspace

struct Layout {
    size_t keys[2], pay[2];     // uint32 [n] each: the sort's ping and pong
    size_t hist, hist_sums;     // the sort's digit tables
    size_t counters;            // uint64 [kCounters]
    size_t tables;              // uint16 [batch, G_0 + G_1]: the count tables of the batch's replicates
    size_t sums;                // uint64 [batch, tiles, 2]: weighted targets and weighted trials per tile, then their scan
    size_t totals;              // uint64 [batch, 2]: P_b and P_b + N_b
    size_t eer, dcf;            // EerCand / DcfCand [batch, tiles]
    size_t below;               // uint64 [batch, tiles]
    size_t total;               // 0: refused
    int32_t batch;
    int64_t tiles;
};

inline bool groups_ok(int64_t g) { return g >= 0 && g <= kMaxGroups; }

inline Layout make_layout(int64_t n, int64_t n_boot, int64_t g_rows, int64_t g_cols) {
    Layout l{};
    l.batch = batch_size(n, n_boot);
    if (!l.batch || !groups_ok(g_rows) || !groups_ok(g_cols)) return Layout{};
    l.tiles = tiles_of(n);
    const size_t hist_len = (size_t)l.tiles * kRadix, cells = (size_t)l.batch * (size_t)l.tiles;
    Carver c;
    for (int i = 0; i < 2; ++i) l.keys[i] = c.take_bytes((size_t)n * 4);
    for (int i = 0; i < 2; ++i) l.pay[i] = c.take_bytes((size_t)n * 4);
    l.hist = c.take_bytes(hist_len * 4);
    l.hist_sums = c.take_bytes((size_t)tiles_of((int64_t)hist_len) * 4);
    l.counters = c.take_bytes(kCounters * 8);
    l.tables = c.take_bytes((size_t)l.batch * (size_t)(g_rows + g_cols) * 2);
    l.sums = c.take_bytes(cells * 16);
    l.totals = c.take_bytes((size_t)l.batch * 16);
    l.eer = c.take_bytes(cells * 24);
    l.dcf = c.take_bytes(cells * 24);
    l.below = c.take_bytes(cells * 8);
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_params(const xvec_boot_params* p, Refusal& why) {
    if (!p) return why.refuse("null pointer: params");
    if (p->n_boot < 1 || p->n_boot > kMaxBoot) return why.refuse("n_boot = %d must lie in 1 .. %d", p->n_boot, kMaxBoot);
    if (p->n_row_groups > kMaxGroups || p->n_col_groups > kMaxGroups)
        return why.refuse("%d row and %d column groups: at most %d on a side", p->n_row_groups, p->n_col_groups, kMaxGroups);
    if ((p->row_group != nullptr) != (p->n_row_groups >= 1) || p->n_row_groups < 0)
        return why.refuse("n_row_groups = %d: at least one group with row_group, 0 without", p->n_row_groups);
    if ((p->col_group != nullptr) != (p->n_col_groups >= 1) || p->n_col_groups < 0)
        return why.refuse("n_col_groups = %d: at least one group with col_group, 0 without", p->n_col_groups);
    if (p->joint && (!p->row_group || !p->col_group))
        return why.refuse("joint needs row_group and col_group");
    if (p->joint && p->n_row_groups != p->n_col_groups)
        return why.refuse("joint needs n_row_groups == n_col_groups (got %d and %d)", p->n_row_groups, p->n_col_groups);
    if (!(p->c_miss >= 0.0) || !(p->c_fa >= 0.0) || !(p->p_target >= 0.0 && p->p_target <= 1.0) || p->c_miss > 1e300 ||
        p->c_fa > 1e300)
        return why.refuse("c_miss = %g and c_fa = %g must be finite and >= 0, p_target = %g in [0, 1]", p->c_miss, p->c_fa,
                          p->p_target);
    return 0;
}

// the plain vector has no sides: groups need index arrays
inline int check_vector_groups(const void* row_idx, const xvec_boot_params* p, Refusal& why) {
    if (!row_idx && (p->row_group || p->col_group))
        return why.refuse("the plain vector form has no groups: its trials are resampled one by one");
    return 0;
}

inline int check_outputs(const void* summary, const void* records, Refusal& why) {
    if (!summary || !records) return why.refuse("null pointer: summary / records");
    return 0;
}

inline int check_host_counts(int32_t b, int32_t side, int32_t n_groups, const void* out, Refusal& why) {
    if (b < 1 || b > kMaxBoot) return why.refuse("b = %d must lie in 1 .. %d", b, kMaxBoot);
    if (side != 0 && side != 1) return why.refuse("side = %d must be 0 (rows) or 1 (columns)", side);
    if (n_groups < 1 || n_groups > kMaxGroups) return why.refuse("n_groups = %d must lie in 1 .. %d", n_groups, kMaxGroups);
    if (!out) return why.refuse("null pointer: counts_out");
    return 0;
}

inline int check_host_poisson(int32_t b, int64_t t, const void* out, Refusal& why) {
    if (b < 1 || b > kMaxBoot) return why.refuse("b = %d must lie in 1 .. %d", b, kMaxBoot);
    if (t < 0 || t >= 0x7fffffff) return why.refuse("t = %lld must lie in 0 .. 2^31 - 2", (long long)t);
    if (!out) return why.refuse("null pointer: weight_out");
    return 0;
}

// What a replicate of P targets and A trials in all (weighted) is: 0 evaluated, 1 degenerate, 2 overflow.  The kernels and the
// CPU test of the overflow rule ask this one function.
XVEC_BOOT_HD int replicate_state(int64_t P, int64_t A) {
    if (A >= kOverflow) return 2;
    return P <= 0 || A - P <= 0 ? 1 : 0;
}

}  // namespace boot_plan
}  // namespace xvec

#undef XVEC_BOOT_HD
#undef XVEC_BOOT_POISSON_TABLE
