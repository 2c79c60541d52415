// The host side of the GMM-UBM unit (csrc/gmm.hip, include/xvec_gmm.h): the argument checks with one text per refusal (the
// utterance ranges among them), the tiles, the slices of the global statistics and the workspace layouts.  Host-compilable (no
// HIP header), so that tests/test_gmm.py can ask it on the CPU (tests/abi/gmm_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_gmm.h"
#include "plan_support.h"

namespace xvec {
namespace gmm_plan {

constexpr int kThreads = 256;
constexpr int kFT = XVEC_GMM_FRAME_TILE;      // frames of a tile of ll, and of a chunk of the statistics
constexpr int kCT = XVEC_GMM_COMP_TILE;       // components of a tile
constexpr int kYT = 64;                       // columns of (1, x, x^2) a block of the statistics kernel owns
constexpr int kKC = 16;                       // K values staged per chunk
constexpr int kLD = 80;                       // LDS row stride in doubles (class_scatter.h: kLD)
constexpr int kMaxC = XVEC_GMM_MAX_C;
constexpr int kMaxD = XVEC_GMM_MAX_D;
constexpr int64_t kMaxUtts = XVEC_GMM_MAX_UTTS;
constexpr int kMaxSlices = XVEC_GMM_MAX_SLICES;
constexpr int kMaxIter = XVEC_GMM_MAX_ITER;
constexpr int kTargetBlocks = 1024;           // blocks of the statistics kernel aimed at (fixed: results do not depend on the device)
constexpr int kMinSliceFrames = 1024;         // a slice the plan chooses is worth at least this many frames
constexpr int64_t kMaxFrames = 2147483647;      // rows of statistics and of scores (M, U)
constexpr int64_t kMaxTotal = (int64_t)1 << 30; // frames of a call: a block of 256 threads per 64 frames, a launch holds 2^32 threads
constexpr int64_t kMaxLaunch = ((int64_t)1 << 32) - 256;   // elements of a launch of one thread per element
constexpr int kEmStateBytes = 64;             // gmm.hip: EmState

inline bool model_ok(int32_t C, int32_t D) { return C >= 1 && C <= kMaxC && D >= 1 && D <= kMaxD; }
inline bool total_ok(int64_t n) { return n >= 0 && n <= kMaxTotal; }
inline bool utts_ok(int64_t u) { return u >= 1 && u <= kMaxUtts; }

inline int32_t k_pad(int32_t D) { return (2 * D + 3) / 4 * 4; }
inline int32_t k_chunks(int32_t D) { return (k_pad(D) + kKC - 1) / kKC; }
inline int32_t comp_tiles(int32_t C) { return (C + kCT - 1) / kCT; }
inline int32_t stat_cols(int32_t D, bool per_utt) { return per_utt ? 1 + D : 1 + 2 * D; }
inline int32_t y_tiles(int32_t D, bool per_utt) { return (stat_cols(D, per_utt) + kYT - 1) / kYT; }
inline int64_t frame_tiles(int64_t n) { return (n + kFT - 1) / kFT; }

// slices of the global statistics: as many as keep kTargetBlocks blocks busy, each worth at least kMinSliceFrames frames
inline int32_t slices_of(int64_t n_total, int32_t C, int32_t D, int32_t asked) {
    if (asked) return asked;
    const int64_t by_blocks = kTargetBlocks / ((int64_t)comp_tiles(C) * y_tiles(D, false));
    const int64_t by_frames = (n_total + kMinSliceFrames - 1) / kMinSliceFrames;
    int64_t s = by_blocks < by_frames ? by_blocks : by_frames;
    if (s < 1) s = 1;
    return (int32_t)(s > kMaxSlices ? kMaxSlices : s);
}
// frames of a slice: a whole number of chunks; slices past the frames are empty and add exact zeros
inline int64_t slice_frames(int64_t n_total, int32_t slices) {
    const int64_t per = (n_total + slices - 1) / slices;
    const int64_t r = (per + kFT - 1) / kFT * kFT;
    return r ? r : kFT;
}
inline size_t slab_doubles(int32_t C, int32_t D, int32_t slices) {
    return (size_t)slices * comp_tiles(C) * y_tiles(D, false) * (kCT * kYT);
}

// ---------------------------------------------------------------- workspaces

struct Layout {
    size_t first, off;               // int64 [U], int64 [U + 1]: the utterances on the device
    size_t P, g;                     // the prepared model
    size_t lse;                      // double [n_total]
    size_t slab;                     // double [slices][comp tiles][y tiles][64][64]
    size_t n, f, s, sums, state;     // the EM's statistics, (llsum, n_frames) and EmState
    size_t total;                    // 0: refused
    int32_t slices;
};

inline void take_frames(Carver& c, Layout& l, int64_t U) {
    l.first = c.take_bytes((size_t)U * 8);
    l.off = c.take_bytes((size_t)(U + 1) * 8);
}
inline void take_model(Carver& c, Layout& l, int32_t C, int32_t D) {
    l.P = c.take_bytes((size_t)C * 2 * D * 8);
    l.g = c.take_bytes((size_t)C * 8);
}

inline Layout loglik_layout(int64_t U, int32_t C, int32_t D) {
    Layout l{};
    if (!utts_ok(U) || !model_ok(C, D)) return l;
    Carver c;
    take_frames(c, l, U);
    take_model(c, l, C, D);
    l.total = c.total();
    return l;
}

inline bool slices_ok(int32_t per_utt, int32_t n_slices) {
    return n_slices >= 0 && n_slices <= kMaxSlices && !(per_utt && n_slices);
}

inline Layout accumulate_layout(int64_t n_total, int64_t U, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices) {
    Layout l{};
    if (!total_ok(n_total) || !utts_ok(U) || !model_ok(C, D) || !slices_ok(per_utt, n_slices)) return l;
    Carver c;
    take_frames(c, l, U);
    take_model(c, l, C, D);
    l.lse = c.take_bytes((size_t)(n_total ? n_total : 1) * 8);
    if (!per_utt) {
        l.slices = slices_of(n_total, C, D, n_slices);
        l.slab = c.take_bytes(slab_doubles(C, D, l.slices) * 8);
    }
    l.total = c.total();
    return l;
}

inline Layout em_layout(int64_t n_total, int64_t U, int32_t C, int32_t D, int32_t n_slices) {
    Layout l = accumulate_layout(n_total, U, C, D, 0, n_slices);
    if (!l.total) return l;
    Carver c;
    c.take_bytes(l.total);
    l.n = c.take_bytes((size_t)C * 8);
    l.f = c.take_bytes((size_t)C * D * 8);
    l.s = c.take_bytes((size_t)C * D * 8);
    l.sums = c.take_bytes(16);
    l.state = c.take_bytes(kEmStateBytes);
    l.total = c.total();
    return l;
}

struct ScoreLayout {
    size_t model, test, total;       // double [M, C D], [U, C D]
};

inline bool score_shape_ok(int64_t M, int64_t U, int32_t C, int32_t D) {
    return model_ok(C, D) && M >= 1 && U >= 1 && M <= kMaxFrames && U <= kMaxFrames;
}

inline ScoreLayout score_layout(int64_t M, int64_t U, int32_t C, int32_t D) {
    ScoreLayout l{};
    if (!score_shape_ok(M, U, C, D)) return l;
    Carver c;
    l.model = c.take_bytes((size_t)M * C * D * 8);
    l.test = c.take_bytes((size_t)U * C * D * 8);
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_model(int32_t C, int32_t D, Refusal& why) {
    if (C < 1 || C > kMaxC) return why.refuse("C = %d must lie in 1 .. %d", C, kMaxC);
    if (D < 1 || D > kMaxD) return why.refuse("D = %d must lie in 1 .. %d", D, kMaxD);
    return 0;
}

// the frames of a call; *n_total = the sum of the counts
inline int check_frames(const xvec_gmm_frames* fr, int32_t D, int64_t* n_total, Refusal& why) {
    if (!fr) return why.refuse("null pointer: frames");
    if (!fr->x) return why.refuse("null pointer: x");
    if (fr->x_type != XVEC_GMM_X_F32 && fr->x_type != XVEC_GMM_X_F64)
        return why.refuse("x_type = %d must be 0 (fp32) or 1 (fp64)", fr->x_type);
    if (fr->reserved != 0) return why.refuse("reserved = %d must be 0", fr->reserved);
    if (fr->rows < 1) return why.refuse("rows = %lld: need at least one row", (long long)fr->rows);
    if (fr->ldx < D) return why.refuse("ldx = %lld is smaller than D = %d", (long long)fr->ldx, D);
    if (fr->n_utts < 1 || fr->n_utts > kMaxUtts)
        return why.refuse("n_utts = %lld must lie in 1 .. %lld", (long long)fr->n_utts, (long long)kMaxUtts);
    if (!fr->utt_first || !fr->utt_count) return why.refuse("null pointer: utt_first / utt_count");
    int64_t total = 0;
    for (int64_t u = 0; u < fr->n_utts; ++u) {
        const int64_t a = fr->utt_first[u], n = fr->utt_count[u];
        if (n < 0) return why.refuse("utt_count[%lld] = %lld is negative", (long long)u, (long long)n);
        if (a < 0 || a > fr->rows || n > fr->rows - a)
            return why.refuse("utterance %lld = rows [%lld, %lld + %lld) leaves the %lld rows", (long long)u, (long long)a, (long long)a,
                              (long long)n, (long long)fr->rows);
        total += n;
        if (total > kMaxTotal) return why.refuse("the utterances hold more than 2^30 frames");
    }
    *n_total = total;
    return 0;
}

inline int check_slices(int32_t per_utt, int32_t n_slices, Refusal& why) {
    if (n_slices < 0 || n_slices > kMaxSlices) return why.refuse("n_slices = %d must lie in 0 .. %d", n_slices, kMaxSlices);
    if (per_utt && n_slices) return why.refuse("n_slices = %d must be 0 in the per-utterance form", n_slices);
    return 0;
}

inline int check_options(const xvec_gmm_mstep_options* o, Refusal& why) {
    if (!o) return why.refuse("null pointer: options");
    if (!(o->reg_covar >= 0.0) || !(o->reg_covar <= 1.7976931348623157e308))
        return why.refuse("reg_covar = %g must be finite and not negative", o->reg_covar);
    if (!(o->var_floor >= 0.0) || !(o->var_floor <= 1.7976931348623157e308))
        return why.refuse("var_floor = %g must be finite and not negative", o->var_floor);
    if (!(o->min_count >= 0.0) || !(o->min_count <= 1.7976931348623157e308))
        return why.refuse("min_count = %g must be finite and not negative", o->min_count);
    return 0;
}

inline int check_em(int32_t max_iter, double tol, Refusal& why) {
    if (max_iter < 1 || max_iter > kMaxIter) return why.refuse("max_iter = %d must lie in 1 .. %d", max_iter, kMaxIter);
    if (!(tol >= 0.0)) return why.refuse("tol = %g must not be negative", tol);
    return 0;
}

inline int check_map(int64_t M, double relevance, Refusal& why) {
    if (M < 1 || M > kMaxFrames) return why.refuse("M = %lld must lie in 1 .. 2^31 - 1", (long long)M);
    if (!(relevance > 0.0) || !(relevance <= 1.7976931348623157e308))
        return why.refuse("relevance = %g must be positive and finite", relevance);
    return 0;
}

inline int check_scores(int64_t M, int64_t U, int64_t ld_s, Refusal& why) {
    if (M < 1 || M > kMaxFrames) return why.refuse("M = %lld must lie in 1 .. 2^31 - 1", (long long)M);
    if (U < 1 || U > kMaxFrames) return why.refuse("U = %lld must lie in 1 .. 2^31 - 1", (long long)U);
    if (ld_s < U) return why.refuse("ld_s = %lld is smaller than U = %lld", (long long)ld_s, (long long)U);
    return 0;
}

inline int check_plan_query(int64_t n_total, int64_t U, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices, const void* out,
                            Refusal& why) {
    if (!total_ok(n_total)) return why.refuse("n_total = %lld must lie in 0 .. 2^30", (long long)n_total);
    if (!utts_ok(U)) return why.refuse("n_utts = %lld must lie in 1 .. %lld", (long long)U, (long long)kMaxUtts);
    if (check_model(C, D, why) || check_slices(per_utt, n_slices, why)) return 1;
    if (!out) return why.refuse("null pointer: out");
    return 0;
}

}  // namespace gmm_plan
}  // namespace xvec
