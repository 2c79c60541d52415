// Waveform resampling: resampy's band-limited sinc interpolation at any ratio, one ratio for the batch or one per row (speed
// perturbation).  C ABI and the arithmetic: include/xvec_resample.h; the tap plan of an output: resample_taps.h.
//   A block of 256 threads owns 256 consecutive outputs of one row, a lane per output.  The input samples the tile can touch --
//   floor(255 * inc) + 1 centres plus nwin / step taps on either side -- are staged in LDS as fp32 (exact for int16) where they
//   number at most 8192 (32 KiB: five blocks per CU); at smaller ratios (below about 0.047 for the 64-zero filter) the lanes read
//   the row through the caches instead.  Each lane walks its left wing, then its right wing, in tap order, with its sum in a
//   register.  The filter table (256 KiB of fp64 for kaiser_best: more than the LDS holds) is read through the caches, the
//   two entries of a tap in one 16-byte read.  At a fixed tap index the lanes read inside one window of `step` entries (up to
//   4 KiB); which lane takes which output of the tile is therefore decided by a sort of the tile's outputs by their table
//   offset (a rank count over 256 keys in LDS, before the staging reuses the buffer): the 64 lanes of a wave then read a
//   quarter of that window, and at ratios with few distinct offsets (1, 2, 1 / 3) one address.  Measured: 44.1 kHz -> 16 kHz
//   took 8.0 ms for 256 x 48 000 outputs with lane = output index and takes 2.5 ms sorted.
// The two table entries of a tap are scaled by the ratio (downsampling) and differenced on the fly: the bits of
// win_s[j] + eta * (win_s[j + 1] - win_s[j]) are those of the package's win_s and delta arrays.  No reduction across lanes, no
// atomics: an output is a function of its row alone, whichever lane computes it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_resample.h"
#include "host_support.h"
#include "resample_taps.h"

// Every operation rounds on its own (include/xvec_resample.h): the outputs are compared with numpy bit for bit, and one fused
// multiply-add in a weight or in the running sum changes them.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using namespace resample_taps;

constexpr int kTile = XVEC_RESAMPLE_TILE;
constexpr int kSpanMax = XVEC_RESAMPLE_SPAN_MAX;
constexpr int32_t kDeadKey = 1 << 22;      // sorts behind every table offset (at most 2^XVEC_RESAMPLE_PRECISION_MAX)
static_assert(kSpanMax >= 2 * kTile && XVEC_RESAMPLE_PRECISION_MAX <= 20 && kTile == 256, "the sort's keys fit 31 bits and the staging buffer");

struct RowPlan {
    RatioPlan r;
    int32_t staged;        // tile_span <= kSpanMax: the row's tiles go through LDS
    int32_t reserved;
};
static_assert(sizeof(RowPlan) == 40, "plan layout");

struct ResampleArgs {
    const void* x;
    const void* lens;
    const RowPlan* plans;
    const double* win;
    void* out;
    void* out_len;
    int64_t ld_in, ld_out, n, out_cols, nwin, tiles;
    int32_t P, per_row, len_i32, out_f64;
};

struct __attribute__((packed, aligned(8))) TablePair {
    double a, b;
};

// Both wings of one output.  x_at(s): sample s of the row as a double.
template <bool ACC64, typename Load>
__device__ __forceinline__ double walk_taps(const TapPlan& p, const RatioPlan& r, const double* __restrict__ win, int32_t jlast,
                                            Load x_at) {
    const double ratio = r.ratio;
    const bool scaled = r.scaled != 0;
    const int32_t step = r.step;
    double acc = 0.0;
    auto tap = [&](int32_t j, double eta, int64_t s) {
        // entries j and j + 1 in one 16-byte read (8-byte aligned); the last entry has no right neighbour: delta = 0
        const TablePair e = *reinterpret_cast<const TablePair*>(win + (j < jlast ? j : jlast - 1));
        double a = j < jlast ? e.a : e.b, b = e.b;
        if (scaled) {
            a = a * ratio;
            b = b * ratio;
        }
        const double w = a + eta * (b - a);
        acc = acc + w * x_at(s);
        if (!ACC64) acc = (double)(float)acc;
    };
    {
        const int32_t i0 = (int32_t)p.i_min, i1 = (int32_t)p.i_max;
#pragma unroll 4
        for (int32_t i = i0; i < i1; ++i) tap(p.off_l + i * step, p.eta_l, p.n0 - i);
    }
    {
        const int32_t k1 = (int32_t)p.k_max;
#pragma unroll 4
        for (int32_t k = 0; k < k1; ++k) tap(p.off_r + k * step, p.eta_r, p.n0 + 1 + k);
    }
    return acc;
}

template <typename X, bool ACC64>
__global__ __launch_bounds__(kTile) void resample_kernel(const ResampleArgs g) {
    __shared__ __attribute__((aligned(16))) float sx[kSpanMax];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / g.tiles, tile = blockIdx.x - b * g.tiles;
    const RowPlan rp = g.plans[g.per_row ? b : 0];
    int64_t len = g.n;
    if (g.lens) len = g.len_i32 ? (int64_t) static_cast<const int32_t*>(g.lens)[b] : static_cast<const int64_t*>(g.lens)[b];
    len = len < 0 ? 0 : (len > g.n ? g.n : len);
    const int64_t n_rule = out_len(len, rp.r.ratio);
    const int64_t n_out = n_rule < g.out_cols ? n_rule : g.out_cols;      // the host has checked int(n * ratio) <= out_cols
    if (tile == 0 && tid == 0) {
        if (g.len_i32) static_cast<int32_t*>(g.out_len)[b] = (int32_t)n_rule;
        else static_cast<int64_t*>(g.out_len)[b] = n_rule;
    }
    const int64_t t0 = tile * kTile;
    int64_t t = t0 + tid;
    const X* __restrict__ row = static_cast<const X*>(g.x) + b * g.ld_in;
    double acc = 0.0;
    if (t0 < n_out) {                                  // the same for every lane of the block
        // Which lane takes which output of the tile: the outputs sorted by their left table offset, so that the 64 lanes of a
        // wave read a quarter of the `step` entries a tap index spans (the right offsets are step minus the left ones: sorted
        // too).  A permutation of the tile: every output keeps its own arithmetic.  Outputs past n_out sort last.
        int32_t* skey = reinterpret_cast<int32_t*>(sx);
        const int32_t off = t < n_out ? plan_output(t, rp.r, g.P, g.nwin, len).off_l : kDeadKey;
        const int32_t mine = off * kTile + tid;
        skey[tid] = mine;
        __syncthreads();
        int32_t rank = 0;
#pragma unroll 8
        for (int u = 0; u < kTile; u += 4) {
            const int4 k = *reinterpret_cast<const int4*>(skey + u);
            rank += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
        }
        skey[kTile + rank] = tid;
        __syncthreads();
        t = t0 + skey[kTile + tid];
        __syncthreads();                               // the staging below writes over the keys
        const int64_t t_last = (t0 + kTile < n_out ? t0 + kTile : n_out) - 1;
        const int64_t taps = max_taps(g.nwin, rp.r.step);
        int64_t lo = (int64_t)((double)t0 * rp.r.inc) - taps + 1, hi = (int64_t)((double)t_last * rp.r.inc) + taps + 1;
        lo = lo < 0 ? 0 : lo;
        hi = hi > len ? len : hi;
        const bool staged = rp.staged && hi - lo <= kSpanMax;
        if (staged) {
            for (int64_t s = lo + tid; s < hi; s += kTile) sx[s - lo] = (float)row[s];
            __syncthreads();
        }
        if (t < n_out) {
            const TapPlan p = plan_output(t, rp.r, g.P, g.nwin, len);
            const int32_t jlast = (int32_t)(g.nwin - 1);
            if (staged) acc = walk_taps<ACC64>(p, rp.r, g.win, jlast, [&](int64_t s) { return (double)sx[(int32_t)(s - lo)]; });
            else acc = walk_taps<ACC64>(p, rp.r, g.win, jlast, [&](int64_t s) { return (double)row[s]; });
        }
    }
    if (t < g.out_cols) {                              // columns past n_out: acc is still 0
        if (g.out_f64) static_cast<double*>(g.out)[b * g.ld_out + t] = acc;
        else static_cast<float*>(g.out)[b * g.ld_out + t] = (float)acc;
    }
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_rerr;

constexpr int64_t kMax = 0x7fffffff;

bool table_ok(int64_t nwin, int32_t precision) {
    return precision >= 0 && precision <= XVEC_RESAMPLE_PRECISION_MAX && nwin >= ((int64_t)1 << precision) + 1 && nwin <= kMax;
}

size_t plan_bytes(int32_t n_ratios) {
    Carver c(nullptr);
    c.take<RowPlan>((size_t)n_ratios);
    return c.total();
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_resample_last_error(void) { return g_rerr.c_str(); }

int64_t xvec_resample_out_len(int64_t n, double ratio) { return n >= 0 && ratio_ok(ratio) ? out_len(n, ratio) : -1; }

int64_t xvec_resample_tile_span(double ratio, int64_t nwin, int32_t precision) {
    if (!ratio_ok(ratio) || !table_ok(nwin, precision)) return -1;
    const RatioPlan r = plan_ratio(ratio, 1 << precision);
    return r.step >= 1 ? tile_span(r, nwin, kTile) : -1;
}

size_t xvec_resample_workspace_bytes(int32_t batch, int32_t n_ratios) {
    return batch >= 1 && (n_ratios == 1 || n_ratios == batch) ? plan_bytes(n_ratios) : 0;
}

int xvec_resample(const void* x, int32_t x_dtype, int64_t ld_in, int32_t batch, int64_t n, const void* lens, int32_t len_dtype,
                  const double* ratios, int32_t n_ratios, const double* win, int64_t nwin, int32_t precision, int32_t acc_mode,
                  void* out, int32_t out_dtype, int64_t ld_out, int64_t out_cols, void* out_len_dev, void* workspace,
                  size_t workspace_bytes, xvec_stream stream) {
    if (batch < 1) return g_rerr.fail(XVEC_ERR_ARG, "batch = %d: need at least one row", batch);
    if (n < 1) return g_rerr.fail(XVEC_ERR_ARG, "n = %lld: need at least one sample", (long long)n);
    if (out_cols < 1) return g_rerr.fail(XVEC_ERR_ARG, "out_cols = %lld: need at least one output column", (long long)out_cols);
    if (n > kMax || out_cols > kMax)
        return g_rerr.fail(XVEC_ERR_TOO_LARGE, "n = %lld and out_cols = %lld must be at most 2^31 - 1", (long long)n, (long long)out_cols);
    if (x_dtype != XVEC_RESAMPLE_X_F32 && x_dtype != XVEC_RESAMPLE_X_I16) return g_rerr.fail(XVEC_ERR_ARG, "x_dtype = %d: 0 (fp32) or 1 (int16)", x_dtype);
    if (out_dtype != XVEC_RESAMPLE_OUT_F32 && out_dtype != XVEC_RESAMPLE_OUT_F64)
        return g_rerr.fail(XVEC_ERR_ARG, "out_dtype = %d: 0 (fp32) or 1 (fp64)", out_dtype);
    if (acc_mode != XVEC_RESAMPLE_ACC_F32 && acc_mode != XVEC_RESAMPLE_ACC_F64)
        return g_rerr.fail(XVEC_ERR_ARG, "acc_mode = %d: 0 (fp32 running sum) or 1 (fp64)", acc_mode);
    if (len_dtype != XVEC_RESAMPLE_LEN_I64 && len_dtype != XVEC_RESAMPLE_LEN_I32)
        return g_rerr.fail(XVEC_ERR_ARG, "len_dtype = %d: 0 (int64) or 1 (int32)", len_dtype);
    if (ld_in < n) return g_rerr.fail(XVEC_ERR_ARG, "ld_in = %lld is smaller than n = %lld", (long long)ld_in, (long long)n);
    if (ld_out < out_cols) return g_rerr.fail(XVEC_ERR_ARG, "ld_out = %lld is smaller than out_cols = %lld", (long long)ld_out, (long long)out_cols);
    if (n_ratios != 1 && n_ratios != batch)
        return g_rerr.fail(XVEC_ERR_ARG, "n_ratios = %d: one ratio for the batch or one per row (batch = %d)", n_ratios, batch);
    if (precision < 0 || precision > XVEC_RESAMPLE_PRECISION_MAX)
        return g_rerr.fail(XVEC_ERR_ARG, "precision = %d must be in 0 .. %d", precision, XVEC_RESAMPLE_PRECISION_MAX);
    if (!table_ok(nwin, precision))
        return g_rerr.fail(XVEC_ERR_ARG, "nwin = %lld: the table needs 2^precision + 1 = %lld .. 2^31 - 1 entries", (long long)nwin,
                           (long long)(((int64_t)1 << precision) + 1));
    if (!x) return g_rerr.fail(XVEC_ERR_ARG, "null pointer: x");
    if (!ratios) return g_rerr.fail(XVEC_ERR_ARG, "null pointer: ratios");
    if (!win) return g_rerr.fail(XVEC_ERR_ARG, "null pointer: win");
    if (!out || !out_len_dev) return g_rerr.fail(XVEC_ERR_ARG, "null pointer: out / out_len");
    if (!workspace) return g_rerr.fail(XVEC_ERR_ARG, "null pointer: workspace");
    const int32_t P = 1 << precision;
    std::vector<RowPlan> plans((size_t)n_ratios);
    for (int32_t b = 0; b < n_ratios; ++b) {
        const double ratio = ratios[b];
        if (!ratio_ok(ratio)) return g_rerr.fail(XVEC_ERR_ARG, "ratios[%d] = %g must be finite and positive", b, ratio);
        RowPlan& rp = plans[(size_t)b];
        rp.r = plan_ratio(ratio, P);
        if (rp.r.step < 1)
            return g_rerr.fail(XVEC_ERR_ARG, "ratios[%d] = %g: step = int(ratio * %d) = %d, need at least 1", b, ratio, P, rp.r.step);
        const int64_t longest = out_len(n, ratio);
        if (longest > out_cols)
            return g_rerr.fail(XVEC_ERR_ARG, "out_cols = %lld is smaller than int(n * ratios[%d]) = %lld", (long long)out_cols, b,
                               (long long)longest);
        rp.staged = tile_span(rp.r, nwin, kTile) <= kSpanMax ? 1 : 0;
        rp.reserved = 0;
    }
    int rc;
    if ((rc = workspace_ok(workspace_bytes, plan_bytes(n_ratios), g_rerr))) return rc;
    const int64_t tiles = (out_cols + kTile - 1) / kTile;
    if (tiles * batch > kMax)
        return g_rerr.fail(XVEC_ERR_TOO_LARGE, "%d rows of %lld columns are %lld tiles: more than 2^31 - 1", batch, (long long)out_cols,
                           (long long)(tiles * batch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (pageable source: the copy is staged before the call returns, as for the op list of xvec_aug_mix)
    const hipError_t e = hipMemcpyAsync(workspace, plans.data(), plans.size() * sizeof(RowPlan), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return g_rerr.fail(XVEC_ERR_HIP, "copying the ratio plans failed: %s", hipGetErrorString(e));
    ResampleArgs g{};
    g.x = x;
    g.lens = lens;
    g.plans = static_cast<const RowPlan*>(workspace);
    g.win = win;
    g.out = out;
    g.out_len = out_len_dev;
    g.ld_in = ld_in;
    g.ld_out = ld_out;
    g.n = n;
    g.out_cols = out_cols;
    g.nwin = nwin;
    g.tiles = tiles;
    g.P = P;
    g.per_row = n_ratios == batch && batch > 1 ? 1 : 0;
    g.len_i32 = len_dtype == XVEC_RESAMPLE_LEN_I32;
    g.out_f64 = out_dtype == XVEC_RESAMPLE_OUT_F64;
    const unsigned grid = (unsigned)(tiles * batch);
    const bool i16 = x_dtype == XVEC_RESAMPLE_X_I16, acc64 = acc_mode == XVEC_RESAMPLE_ACC_F64;
    if (i16 && acc64) resample_kernel<int16_t, true><<<grid, kTile, 0, s>>>(g);
    else if (i16) resample_kernel<int16_t, false><<<grid, kTile, 0, s>>>(g);
    else if (acc64) resample_kernel<float, true><<<grid, kTile, 0, s>>>(g);
    else resample_kernel<float, false><<<grid, kTile, 0, s>>>(g);
    return g_rerr.launch_ok("resample_kernel");
}

}  // extern "C"
