// The host side of exact t-SNE (csrc/tsne.hip, include/xvec_tsne.h): the argument checks, the workspace layout and the
// row-group / column-slice plan of the pair pass.  Host-compilable (no HIP header, like diar_plan.h and vad_plan.h), so that
// tests/test_tsne.py can ask it on the CPU (tests/abi/tsne_plan_dump.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_tsne.h"
#include "plan_support.h"

namespace xvec {
namespace tsne_plan {

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_points(int32_t n, Refusal& why) {
    if (n < 2) return why.refuse("n = %d: need at least two points", n);
    if (n > XVEC_TSNE_MAX_POINTS)
        return why.refuse("n = %d is over XVEC_TSNE_MAX_POINTS = %d", n, XVEC_TSNE_MAX_POINTS);
    return 0;
}

// A matrix of doubles with `cols` columns used per row.
inline int check_matrix(const void* p, int64_t ld, int64_t cols, const char* what, Refusal& why) {
    if (!p) return why.refuse("null pointer: %s", what);
    if (reinterpret_cast<uintptr_t>(p) % 8 != 0) return why.refuse("%s is not 8-byte aligned", what);
    if (ld < cols)
        return why.refuse("%s row stride %lld is smaller than its %lld columns", what, (long long)ld, (long long)cols);
    return 0;
}

inline int check_x(const void* x, int32_t x_dtype, int32_t d, int64_t ldx, Refusal& why) {
    if (x_dtype != XVEC_TSNE_X_F32 && x_dtype != XVEC_TSNE_X_F64) return why.refuse("unknown x_dtype %d", x_dtype);
    if (d < 1 || d > XVEC_TSNE_MAX_DIM) return why.refuse("d = %d must lie in 1 .. XVEC_TSNE_MAX_DIM = %d", d, XVEC_TSNE_MAX_DIM);
    if (!x) return why.refuse("null pointer: x");
    const unsigned size = x_dtype == XVEC_TSNE_X_F32 ? 4 : 8;
    if (reinterpret_cast<uintptr_t>(x) % size != 0) return why.refuse("x is not %u-byte aligned", size);
    if (ldx < d) return why.refuse("x row stride %lld is smaller than d = %d", (long long)ldx, d);
    return 0;
}

inline int check_perplexity(double perplexity, int32_t n, Refusal& why) {
    if (!std::isfinite(perplexity) || !(perplexity > 0.0) || !(perplexity < (double)n))
        return why.refuse("perplexity = %g must be finite, positive and below n = %d", perplexity, n);
    return 0;
}

inline int check_steps(int32_t n_components, int32_t n_steps, double exaggeration, double momentum, double learning_rate,
                       double min_gain, Refusal& why) {
    if (n_components != 2) return why.refuse("n_components = %d: only two output dimensions", n_components);
    if (n_steps < 1) return why.refuse("n_steps = %d: need at least one iteration", n_steps);
    if (!std::isfinite(exaggeration) || !(exaggeration > 0.0))
        return why.refuse("exaggeration = %g must be finite and positive", exaggeration);
    if (!std::isfinite(momentum) || momentum < 0.0) return why.refuse("momentum = %g must be finite and not negative", momentum);
    if (!std::isfinite(learning_rate) || !(learning_rate > 0.0))
        return why.refuse("learning_rate = %g must be finite and positive", learning_rate);
    if (!std::isfinite(min_gain) || min_gain < 0.0) return why.refuse("min_gain = %g must be finite and not negative", min_gain);
    return 0;
}

// ---------------------------------------------------------------- the pair pass: row groups and column slices

// Block (g, s) of the pair pass takes rows g * rows .. min(n, (g + 1) * rows) - 1 and columns s * slice_cols ..
// min(n, (s + 1) * slice_cols) - 1.  slice_cols is a multiple of XVEC_TSNE_SLICE_STEP (a slice starts on a 1 KiB boundary of
// its row of P) and at most XVEC_TSNE_SLICE_MAX (its y fits the block's LDS).
struct Plan {
    int32_t rows, slices, slice_cols, groups;
};

inline int32_t ceil_div(int32_t a, int32_t b) { return (a + b - 1) / b; }

// The most slices any device gets: what the workspace is sized by, so that its layout does not depend on the device.
inline int32_t max_slices(int32_t n) { return ceil_div(n, XVEC_TSNE_SLICE_STEP); }

// Rows: the tallest group (a slice's y is staged once per block) that still leaves two blocks per compute unit at the fewest
// slices.  Slices: as many as four blocks per compute unit ask for, between what XVEC_TSNE_SLICE_MAX forces and what
// XVEC_TSNE_SLICE_STEP allows.
inline Plan make_plan(int32_t n, int32_t cus) {
    if (cus < 1) cus = 1;
    const int32_t least = ceil_div(n, XVEC_TSNE_SLICE_MAX);
    int32_t rows = XVEC_TSNE_ROWS_MAX;
    while (rows > XVEC_TSNE_ROWS_MIN && (int64_t)ceil_div(n, rows) * least < 2 * (int64_t)cus) rows /= 2;
    const int32_t groups = ceil_div(n, rows);
    int64_t want = (4 * (int64_t)cus + groups - 1) / groups;
    if (want < least) want = least;
    if (want > max_slices(n)) want = max_slices(n);
    int32_t cols = ceil_div(n, (int32_t)want);
    cols = ceil_div(cols, XVEC_TSNE_SLICE_STEP) * XVEC_TSNE_SLICE_STEP;
    return Plan{rows, ceil_div(n, cols), cols, groups};
}

// Blocks of the update launch: a thread per row.
inline int32_t update_blocks(int32_t n) { return ceil_div(n, XVEC_TSNE_THREADS); }

// ---------------------------------------------------------------- workspace

// Byte offsets of the workspace's parts (each 256-byte aligned).
struct Layout {
    size_t x64;        // double [n, d]: the rows of x widened (xvec_tsne_sqdist)
    size_t sqnorm;     // double [n]: |x_i|^2
    size_t row_sum;    // double [n]: the rows' sums of C (xvec_tsne_affinities)
    size_t scalars;    // double [4]: sum C, Z, and two spare
    size_t partials;   // double [max_slices(n), n, 5]: the pair pass's sums, [slice][row][5]
    size_t kl_part;    // double [max_slices(n), n]: the KL pass's sums
    size_t norm_part;  // double [update_blocks(n)]: the update blocks' sums of grad^2
    size_t total;
};

inline Layout make_layout(int32_t n, int32_t d) {
    Layout l{};
    Carver c;
    const size_t N = (size_t)n, S = (size_t)max_slices(n);
    l.x64 = c.take_bytes(N * (size_t)d * sizeof(double));
    l.sqnorm = c.take_bytes(N * sizeof(double));
    l.row_sum = c.take_bytes(N * sizeof(double));
    l.scalars = c.take_bytes(4 * sizeof(double));
    l.partials = c.take_bytes(S * N * 5 * sizeof(double));
    l.kl_part = c.take_bytes(S * N * sizeof(double));
    l.norm_part = c.take_bytes((size_t)update_blocks(n) * sizeof(double));
    l.total = c.total();
    return l;
}

static_assert(XVEC_TSNE_THREADS * XVEC_TSNE_ROW_ITEMS >= XVEC_TSNE_MAX_POINTS, "a block's registers hold a row of distances");
static_assert(XVEC_TSNE_SLICE_MAX % XVEC_TSNE_SLICE_STEP == 0 && XVEC_TSNE_SLICE_STEP == 2 * 64, "a wave reads a step per load");
static_assert(XVEC_TSNE_ROWS_MIN % 4 == 0, "four waves share a group's rows");

}  // namespace tsne_plan
}  // namespace xvec
