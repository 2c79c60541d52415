// Score normalisation against a cohort: per-row mean and standard deviation of the K largest cells of an fp64 score matrix
// (Z-, T-, S-, AS-norm), and the normalisation itself.  C ABI and the definitions: include/xvec_snorm.h.
//   row stats   one block of 512 threads per row.  The cells become order-preserving 64-bit keys (snorm_keys.h); the k-th
//               largest key is found by a radix select, most significant digit first: eight passes, each a 256-bin histogram
//               in LDS of the keys that still share the chosen prefix, a suffix scan of the bins, one digit chosen.  Then
//               sum x over the keys above the cut + (k - above) * cut value, the mean, and a second pass sum (x - mean)^2.
//               RESIDENT rows (C <= 16384): read from memory once, the keys stay in LDS through all ten passes.
//               STREAMED rows (longer ones; top_k = 0 beyond 4096 cells): every pass reads the row again (from L2 where it
//               fits) and keys it on the fly.  top_k = 0 takes every valid cell: no select, three passes.
//   apply       out = w (s - mr) / sr + w (s - mc) / sc, tiles of 8 rows x 256 columns, a thread per column.
// Only integer counts go through (LDS) atomics; every floating-point sum has one fixed order: thread t adds its cells
// t, t + 512, ... in that order, the 64 lanes of a wave combine in a butterfly, the eight waves' sums are added in wave order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_snorm.h"
#include "host_support.h"
#include "snorm_keys.h"
#include "trial_device.h"

// Every operation rounds on its own: the error bounds of tests/test_snorm_gpu.py count roundings, and apply's symmetry
// (include/xvec_snorm.h) does not survive a multiply-add fused on one side of the sum only.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using namespace snorm_keys;
using trial_device::block_sum;      // the sum order of the last line above, over the kWaves doubles handed to it

constexpr int kThreads = XVEC_SNORM_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kResidentSmall = XVEC_SNORM_RESIDENT_SMALL;
constexpr int kResidentMax = XVEC_SNORM_RESIDENT_MAX;
constexpr int kStreamLoadAhead = 8;           // loads of a streamed row a thread has in flight in the first pass
constexpr int kAhead = 4;                     // keys a thread fetches ahead of their use in the later passes
constexpr int kApplyRows = XVEC_SNORM_APPLY_ROWS;
constexpr int kApplyCols = XVEC_SNORM_APPLY_COLS;
static_assert(kRadix <= kThreads && kRadix % 64 == 0, "one thread per histogram bin, whole waves");
static_assert(sizeof(xvec_snorm_select_record) == 16, "record layout");

struct RowStatsArgs {
    const double* scores;
    int64_t ld;
    uint32_t C, top_k;
    const int32_t* skip_col;
    double *mean, *std, *kth;
    int32_t* n_used;
    xvec_snorm_select_record* rec;
};

// ---------------------------------------------------------------- row statistics

// CAP > 0: resident, the row's keys in CAP words of LDS.  CAP == 0: streamed.
template <int CAP>
__global__ __launch_bounds__(kThreads) void snorm_row_stats_kernel(const RowStatsArgs g) {
    __shared__ uint64_t skey[CAP > 0 ? CAP : 1];
    __shared__ double wsum[kWaves];
    __shared__ uint32_t hist[kRadix];
    __shared__ uint32_t wtot[kRadix / 64];
    __shared__ uint32_t sel[2];               // the chosen digit, k inside it
    __shared__ uint32_t s_valid, s_ties;
    __shared__ unsigned long long s_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t C = g.C;
    const int64_t row_i = blockIdx.x;
    const double* __restrict__ row = g.scores + row_i * g.ld;
    const uint32_t skip = g.skip_col ? (uint32_t)g.skip_col[row_i] : 0xffffffffu;      // -1 -> no column

    // the key of cell j (kKeyVoid: takes no part)
    auto key_at = [&](uint32_t j) -> uint64_t { return CAP > 0 ? skey[j] : cell_key(row[j], j == skip); };

    if (tid < kRadix) hist[tid] = 0;
    if (tid == 0) {
        s_valid = s_ties = 0;
        s_min = ~0ull;
    }
    __syncthreads();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // resident: every load of the row is in flight at once (CAP / 512 per thread); streamed: kStreamLoadAhead at a time
    constexpr int kLoadAhead = CAP > 0 ? CAP / kThreads : kStreamLoadAhead;
    {   // valid cells and the smallest key; resident: the one read of the row
        uint32_t mine = 0;
        unsigned long long lo = ~0ull;
        for (uint32_t j0 = 0; j0 < C; j0 += kLoadAhead * kThreads) {
            double x[kLoadAhead];
#pragma unroll
            for (int u = 0; u < kLoadAhead; ++u) {
                const uint32_t j = j0 + u * kThreads + tid;
                x[u] = j < C ? row[j] : nan;
            }
#pragma unroll
            for (int u = 0; u < kLoadAhead; ++u) {
                const uint32_t j = j0 + u * kThreads + tid;
                const uint64_t key = cell_key(x[u], j == skip);
                if (CAP > 0 && j < C) skey[j] = key;
                if (key != kKeyVoid) {
                    ++mine;
                    lo = key < lo ? key : lo;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            mine += __shfl_xor(mine, off);
            const unsigned long long y = __shfl_xor(lo, off);
            lo = y < lo ? y : lo;
        }
        if (lane == 0 && mine) {
            atomicAdd(&s_valid, mine);
            atomicMin(&s_min, lo);
        }
    }
    __syncthreads();
    const uint32_t v = s_valid;
    const uint32_t k = g.top_k == 0 ? v : (g.top_k < v ? g.top_k : v);
    // every valid cell is taken: no walk, the cut is the smallest key and the cells that have it are counted beside the sum
    const bool all_taken = k == v;

    // the keys of the thread's next kAhead cells (t, t + 512, ... from j0 on), fetched before any of them is used
    auto fetch = [&](uint32_t j0, uint64_t (&key)[kAhead]) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const uint32_t j = j0 + u * kThreads + tid;
            key[u] = j < C ? key_at(j) : kKeyVoid;
        }
    };

    uint64_t prefix = all_taken ? s_min : 0;
    uint32_t k_in = k;                        // the k_in-th largest of the keys that share the prefix
    if (k >= 1 && !all_taken) {               // radix select of the k-th largest key
        for (int pass = 0; pass < kPasses; ++pass) {
            for (uint32_t j0 = 0; j0 < C; j0 += kAhead * kThreads) {
                uint64_t key[kAhead];
                fetch(j0, key);
#pragma unroll
                for (int u = 0; u < kAhead; ++u)      // integer counts: the order of the atomics cannot matter
                    if (key[u] != kKeyVoid && in_prefix(key[u], prefix, pass)) atomicAdd(&hist[digit_of(key[u], pass)], 1u);
            }
            __syncthreads();
            // thread t < 256 owns digit 255 - t: an inclusive scan in thread order counts the keys with that digit or a larger one
            uint32_t cnt = 0, incl = 0;
            if (tid < kRadix) {
                cnt = incl = hist[kRadix - 1 - tid];
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = __shfl_up(incl, off);
                    if (lane >= off) incl += y;
                }
                if (lane == 63) wtot[wave] = incl;
            }
            __syncthreads();
            if (tid < kRadix) {
                uint32_t above = incl - cnt;
                for (int w = 0; w < wave; ++w) above += wtot[w];
                if (digit_holds_kth(above, cnt, k_in)) {      // exactly one thread
                    sel[0] = (uint32_t)(kRadix - 1 - tid);
                    sel[1] = k_in - above;
                }
                hist[kRadix - 1 - tid] = 0;                   // for the next pass
            }
            __syncthreads();
            prefix = (prefix << kDigitBits) | sel[0];
            k_in = sel[1];
        }
    }
    // prefix = the cut key; k_in of the cells AT the cut are taken, the k - k_in cells above it all are
    const uint64_t cut = prefix;
    const double cut_value = value_of_key(cut);
    double mean = nan, sd = nan;
    if (k >= 2) {
        double acc = 0.0;
        uint32_t at_cut = 0;
        for (uint32_t j0 = 0; j0 < C; j0 += kAhead * kThreads) {
            uint64_t key[kAhead];
            fetch(j0, key);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (key[u] > cut) acc += value_of_key(key[u]);
                at_cut += key[u] == cut;
            }
        }
        if (all_taken) {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) at_cut += __shfl_xor(at_cut, off);
            if (lane == 0 && at_cut) atomicAdd(&s_ties, at_cut);
        }
        const double sum = block_sum(acc, wsum);
        if (all_taken) k_in = s_ties;
        const double ties = (double)k_in;
        // no cell above the cut: the selection is k copies of one value, whose mean is that value and not fl(fl(k x) / k)
        mean = k_in == k ? cut_value : (sum + ties * cut_value) / (double)k;
        acc = 0.0;
        for (uint32_t j0 = 0; j0 < C; j0 += kAhead * kThreads) {
            uint64_t key[kAhead];
            fetch(j0, key);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (key[u] > cut) {
                    const double d = value_of_key(key[u]) - mean;
                    acc += d * d;
                }
            }
        }
        const double dc = cut_value - mean;
        sd = sqrt((block_sum(acc, wsum) + ties * (dc * dc)) / (double)(k - 1));
    }
    if (tid == 0) {
        g.mean[row_i] = mean;
        g.std[row_i] = sd;
        g.kth[row_i] = k >= 2 ? cut_value : nan;
        g.n_used[row_i] = (int32_t)k;
        xvec_snorm_select_record r;
        r.cut_key = k >= 1 ? cut : 0;
        r.n_above = k - (k >= 1 ? k_in : 0);
        r.n_valid = v;
        g.rec[row_i] = r;
    }
}

// ---------------------------------------------------------------- apply

struct ApplyArgs {
    const double* scores;
    double* out;
    int64_t ld, ld_out, n_rows, n_cols, col_tiles;
    const double *row_mean, *row_std, *col_mean, *col_std;
};

__global__ __launch_bounds__(kApplyCols) void snorm_apply_kernel(const ApplyArgs g) {
    const int64_t tile_r = blockIdx.x / g.col_tiles, tile_c = blockIdx.x - tile_r * g.col_tiles;
    const int64_t j = tile_c * kApplyCols + threadIdx.x;
    if (j >= g.n_cols) return;
    const bool rows = g.row_mean != nullptr, cols = g.col_mean != nullptr;
    const double w = rows && cols ? 0.5 : 1.0;
    const double mc = cols ? g.col_mean[j] : 0.0, sc = cols ? g.col_std[j] : 1.0;
    const int64_t i0 = tile_r * kApplyRows;
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r) {
        const int64_t i = i0 + r;
        if (i >= g.n_rows) break;
        const double s = g.scores[i * g.ld + j];
        double o;
        if (rows) {
            const double tr = w * ((s - g.row_mean[i]) / g.row_std[i]);
            o = cols ? tr + w * ((s - mc) / sc) : tr;
        } else {
            o = w * ((s - mc) / sc);
        }
        g.out[i * g.ld_out + j] = o;
    }
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_nerr;

bool shape_ok(int64_t n, int64_t C) { return n >= 1 && C >= 1 && n <= 0x7fffffff && C <= 0x7fffffff; }

size_t record_bytes(int64_t n) {
    Carver c(nullptr);
    c.take<xvec_snorm_select_record>((size_t)n);
    return c.total();
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_snorm_last_error(void) { return g_nerr.c_str(); }

size_t xvec_snorm_workspace_bytes(int64_t n, int64_t C) { return shape_ok(n, C) ? record_bytes(n) : 0; }

int xvec_snorm_row_stats(const double* scores, int64_t ld, int64_t n, int64_t C, int64_t top_k, const int32_t* skip_col,
                         double* mean, double* std, double* kth, int32_t* n_used, void* workspace, size_t workspace_bytes,
                         xvec_stream stream) {
    if (n < 1) return g_nerr.fail(XVEC_ERR_ARG, "n = %lld: need at least one row", (long long)n);
    if (C < 1) return g_nerr.fail(XVEC_ERR_ARG, "C = %lld: need at least one cohort column", (long long)C);
    if (n > 0x7fffffff || C > 0x7fffffff)
        return g_nerr.fail(XVEC_ERR_TOO_LARGE, "cohort score matrix [%lld, %lld]: both sizes must be at most 2^31 - 1", (long long)n,
                           (long long)C);
    if (ld < C) return g_nerr.fail(XVEC_ERR_ARG, "ld = %lld is smaller than C = %lld", (long long)ld, (long long)C);
    if (top_k < 0) return g_nerr.fail(XVEC_ERR_ARG, "top_k = %lld must not be negative (0 = every valid cell)", (long long)top_k);
    if (!scores) return g_nerr.fail(XVEC_ERR_ARG, "null pointer: scores");
    if (!mean || !std || !kth || !n_used) return g_nerr.fail(XVEC_ERR_ARG, "null pointer: mean / std / kth / n_used");
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, record_bytes(n), g_nerr))) return rc;
    RowStatsArgs g{};
    g.scores = scores;
    g.ld = ld;
    g.C = (uint32_t)C;
    g.top_k = (uint32_t)(top_k < C ? top_k : C);      // k = min(top_k, v) and v <= C
    g.skip_col = skip_col;
    g.mean = mean;
    g.std = std;
    g.kth = kth;
    g.n_used = n_used;
    g.rec = static_cast<xvec_snorm_select_record*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)n;
    // The three kernels give the same bits for the same row (same cells per thread, same order of the sums): which one runs
    // is a matter of speed.  top_k = 0 takes every valid cell and needs three passes, not ten: beyond the small image it is
    // faster to read the row again from L2 at four blocks per CU than to hold it in LDS at one.
    if (C <= kResidentSmall) snorm_row_stats_kernel<kResidentSmall><<<grid, kThreads, 0, s>>>(g);
    else if (C <= kResidentMax && top_k != 0) snorm_row_stats_kernel<kResidentMax><<<grid, kThreads, 0, s>>>(g);
    else snorm_row_stats_kernel<0><<<grid, kThreads, 0, s>>>(g);
    return g_nerr.launch_ok("snorm_row_stats_kernel");
}

int xvec_snorm_apply(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const double* row_mean,
                     const double* row_std, const double* col_mean, const double* col_std, double* out, int64_t ld_out,
                     xvec_stream stream) {
    if (n_rows < 1 || n_cols < 1 || n_rows > 0x7fffffff || n_cols > 0x7fffffff)
        return g_nerr.fail(XVEC_ERR_ARG, "score matrix [%lld, %lld]: both sizes must be in 1 .. 2^31 - 1", (long long)n_rows,
                           (long long)n_cols);
    if (ld < n_cols || ld_out < n_cols)
        return g_nerr.fail(XVEC_ERR_ARG, "ld = %lld and ld_out = %lld must be at least n_cols = %lld", (long long)ld,
                           (long long)ld_out, (long long)n_cols);
    if (!scores || !out) return g_nerr.fail(XVEC_ERR_ARG, "null pointer: scores / out");
    if ((row_mean == nullptr) != (row_std == nullptr) || (col_mean == nullptr) != (col_std == nullptr))
        return g_nerr.fail(XVEC_ERR_ARG, "a mean and its std must both be given or both be null");
    if (!row_mean && !col_mean) return g_nerr.fail(XVEC_ERR_ARG, "neither row nor column statistics: nothing to normalise with");
    if (out == scores && ld_out != ld)
        return g_nerr.fail(XVEC_ERR_ARG, "in place (out == scores) needs ld_out == ld (got %lld and %lld)", (long long)ld_out,
                           (long long)ld);
    ApplyArgs g{};
    g.scores = scores;
    g.out = out;
    g.ld = ld;
    g.ld_out = ld_out;
    g.n_rows = n_rows;
    g.n_cols = n_cols;
    g.col_tiles = (n_cols + kApplyCols - 1) / kApplyCols;
    g.row_mean = row_mean;
    g.row_std = row_std;
    g.col_mean = col_mean;
    g.col_std = col_std;
    const int64_t tiles = g.col_tiles * ((n_rows + kApplyRows - 1) / kApplyRows);
    if (tiles > 0x7fffffff)
        return g_nerr.fail(XVEC_ERR_TOO_LARGE, "%lld x %lld cells are %lld tiles: more than 2^31 - 1", (long long)n_rows,
                           (long long)n_cols, (long long)tiles);
    snorm_apply_kernel<<<(unsigned)tiles, kApplyCols, 0, static_cast<hipStream_t>(stream)>>>(g);
    return g_nerr.launch_ok("snorm_apply_kernel");
}

}  // extern "C"
