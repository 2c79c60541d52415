// Score analysis: moments and histograms of the trial scores, and the hardest trials of either class.
// C ABI and the definitions: include/xvec_analyze.h.  Plan, checks, the bin map and the layouts: analyze_plan.h.  The trial
// reader and the block primitives: trial_device.h; the fp64 key and the digit walk: snorm_keys.h.  Every kernel that reads
// trials runs on the persistent grid of the plan: block b walks the tiles [first_tile(b), first_tile(b + 1)) in rising order.
//   summary   pass 1     n, min, max with their trial indices, the sum, the histogram; a partial per block
//             merge 1    one block: the partials in the plan's order, mean, the class "all"
//             pass 2     M2 about the means; a partial per block
//             merge 2    one block: var
//   hardest   digit      per digit pass (launched kPasses times; a pass returns at once when both classes are settled): the
//                        histogram of the digit among the trials that carry the prefix chosen so far
//             walk       one block: which digit holds the k-th key, and whether bucket and everything above fit the candidates
//             count      per block: trials above the prefix and trials in it, per class
//             offsets    one block: the scan of those counts
//             write      the order-preserving compaction into the candidate buffers: the trials above first, then the bucket's
//             final      one block per class: the rest of the walk over the candidates, the survivors ordered in LDS, the records
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/xvec_analyze.h"
#include "../../include/xvec_hip.h"
#include "analyze_plan.h"
#include "host_support.h"
#include "snorm_keys.h"
#include "trial_device.h"
#include "trial_plan.h"

namespace xvec {
namespace {

using namespace trial_device;
using namespace analyze_plan;

struct AnArgs {
    TrialArgs trials;
    int upper_only;                        // all pairs only
    int64_t tiles, blocks;
};

// The reader of every kernel here: trial_device's, and behind it the predicate of upper_only.
template <bool ALL_PAIRS>
__device__ __forceinline__ Trial take_trial(const AnArgs& g, int64_t t) {
    Trial r = read_trial<ALL_PAIRS>(g.trials, t);
    if (ALL_PAIRS && g.upper_only && r.row >= r.col) r.what = kSkip;
    return r;
}

// a[c] of a two-element array by selection: an index that is not a constant would put the array in memory
template <typename T>
__device__ __forceinline__ T sel(const T (&a)[2], int c) {
    return c ? a[1] : a[0];
}

// ================================================================ summary

struct Part1 {
    long long n[2];
    double sum[2];
    double mn[2];
    long long tmn[2];
    double mx[2];
    long long tmx[2];
    long long n_nan, n_bad;
};
static_assert(sizeof(Part1) == kPart1Bytes, "analyze_plan.h: kPart1Bytes");
struct Part2 {
    double m2[2];
};
static_assert(sizeof(Part2) == kPart2Bytes, "analyze_plan.h: kPart2Bytes");

// An extreme and the lowest trial index that attains it; t < 0: none yet.
struct Ext {
    double v;
    long long t;
};
template <bool MIN>
__device__ __forceinline__ Ext ext_best(Ext a, Ext b) {
    const bool b_wins = b.t >= 0 && (a.t < 0 || (MIN ? b.v < a.v : b.v > a.v) || (b.v == a.v && b.t < a.t));
    Ext r;                                 // field by field: a choice between the two objects would put them in memory
    r.v = b_wins ? b.v : a.v;
    r.t = b_wins ? b.t : a.t;
    return r;
}
template <bool MIN>
__device__ __forceinline__ Ext block_ext(Ext e, Ext (&wbuf)[kWaves]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Ext o;
        o.v = __shfl_xor(e.v, off);
        o.t = __shfl_xor(e.t, off);
        e = ext_best<MIN>(e, o);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wbuf[threadIdx.x >> 6] = e;
    __syncthreads();
    Ext s = wbuf[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s = ext_best<MIN>(s, wbuf[w]);
    return s;
}

struct HistArgs {
    double width;
    long long first;
    int32_t n_bins, rounding, copies;
    unsigned long long* counts;            // [2][n_bins + 2], cleared before the pass
};

template <bool ALL_PAIRS, bool HIST>
__global__ __launch_bounds__(kThreads) void analyze_pass1_kernel(const AnArgs g, const HistArgs h, Part1* parts) {
    __shared__ uint32_t table[HIST ? kHistWords : 1];
    __shared__ double wd[kWaves];
    __shared__ long long wl[kWaves];
    __shared__ Ext we[kWaves];
    const int32_t slots = 2 * (h.n_bins + 2), stride = copy_stride(slots);
    if (HIST) {
        for (int i = threadIdx.x; i < h.copies * stride; i += kThreads) table[i] = 0;
        __syncthreads();
    }
    uint32_t* const mine = table + (HIST ? (threadIdx.x & (h.copies - 1)) * stride : 0);
    long long n0 = 0, n1 = 0, n_nan = 0, n_bad = 0;
    double s0 = 0.0, s1 = 0.0;
    Ext mn0{0.0, -1}, mn1{0.0, -1}, mx0{0.0, -1}, mx1{0.0, -1};
    const int64_t t0 = first_tile(blockIdx.x, g.tiles, g.blocks), t1 = first_tile(blockIdx.x + 1, g.tiles, g.blocks);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t base = tile * kTile + threadIdx.x;
        Trial tr[kItems];
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int64_t t = base + j * kThreads;
            if (t < g.trials.n) tr[j] = take_trial<ALL_PAIRS>(g, t); else tr[j].what = kSkip;
        }
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int64_t t = base + j * kThreads;
            n_nan += tr[j].what == kNan;
            n_bad += tr[j].what == kBad;
            if (tr[j].what != kUse) continue;
            const double s = tr[j].score;
            if (tr[j].target) {
                ++n1;
                s1 += s;
                if (mn1.t < 0 || s < mn1.v) mn1 = Ext{s, t};      // t rises: the first to attain it stays
                if (mx1.t < 0 || s > mx1.v) mx1 = Ext{s, t};
            } else {
                ++n0;
                s0 += s;
                if (mn0.t < 0 || s < mn0.v) mn0 = Ext{s, t};
                if (mx0.t < 0 || s > mx0.v) mx0 = Ext{s, t};
            }
            if (HIST) atomicAdd(&mine[(tr[j].target ? h.n_bins + 2 : 0) + slot_of(s, h.width, h.first, h.n_bins, h.rounding)], 1u);
        }
    }
    n0 = block_count(n0, wl);
    n1 = block_count(n1, wl);
    n_nan = block_count(n_nan, wl);
    n_bad = block_count(n_bad, wl);
    s0 = block_sum(s0, wd);
    s1 = block_sum(s1, wd);
    const Ext a0 = block_ext<true>(mn0, we), a1 = block_ext<true>(mn1, we);
    const Ext b0 = block_ext<false>(mx0, we), b1 = block_ext<false>(mx1, we);
    if (threadIdx.x == 0) {
        Part1& p = parts[blockIdx.x];
        p.n[0] = n0, p.n[1] = n1, p.n_nan = n_nan, p.n_bad = n_bad;
        p.sum[0] = s0, p.sum[1] = s1;
        p.mn[0] = a0.v, p.tmn[0] = a0.t, p.mn[1] = a1.v, p.tmn[1] = a1.t;
        p.mx[0] = b0.v, p.tmx[0] = b0.t, p.mx[1] = b1.v, p.tmx[1] = b1.t;
    }
    if (HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += kThreads) {
            unsigned long long c = 0;
            for (int k = 0; k < h.copies; ++k) c += table[k * stride + i];
            if (c) atomicAdd(&h.counts[i], c);
        }
    }
}

__device__ __forceinline__ double nan_value() { return __longlong_as_double(0x7ff8000000000000ll); }

// mean = sum / n, moved into [lo, hi] where rounding put it outside (a NaN stays)
__device__ __forceinline__ double mean_of(double sum, long long n, double lo, double hi) {
    double m = sum / (double)n;
    if (m < lo) m = lo;
    if (m > hi) m = hi;
    return m;
}

// one class of the output from its merged partials (var comes with pass 2)
__device__ __forceinline__ void write_class(xvec_analyze_class& k, long long n, double sum, const Ext& mn, const Ext& mx) {
    k.n = n;
    k.t_min = mn.t;
    k.t_max = mx.t;
    k.min = n ? mn.v : nan_value();
    k.max = n ? mx.v : nan_value();
    k.sum = n ? sum : nan_value();
    k.mean = n ? mean_of(sum, n, mn.v, mx.v) : nan_value();
    k.var = nan_value();
}

__global__ __launch_bounds__(kThreads) void analyze_merge1_kernel(const Part1* parts, int blocks, xvec_analyze_stats* out) {
    __shared__ double wd[kWaves];
    __shared__ long long wl[kWaves];
    __shared__ Ext we[kWaves];
    long long n0 = 0, n1 = 0, n_nan = 0, n_bad = 0;
    double s0 = 0.0, s1 = 0.0;
    Ext mn0{0.0, -1}, mn1{0.0, -1}, mx0{0.0, -1}, mx1{0.0, -1};
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        const Part1& p = parts[b];
        n_nan += p.n_nan;
        n_bad += p.n_bad;
        n0 += p.n[0];
        n1 += p.n[1];
        s0 += p.sum[0];
        s1 += p.sum[1];
        mn0 = ext_best<true>(mn0, Ext{p.mn[0], p.tmn[0]});
        mn1 = ext_best<true>(mn1, Ext{p.mn[1], p.tmn[1]});
        mx0 = ext_best<false>(mx0, Ext{p.mx[0], p.tmx[0]});
        mx1 = ext_best<false>(mx1, Ext{p.mx[1], p.tmx[1]});
    }
    n_nan = block_count(n_nan, wl);
    n_bad = block_count(n_bad, wl);
    n0 = block_count(n0, wl);
    n1 = block_count(n1, wl);
    s0 = block_sum(s0, wd);
    s1 = block_sum(s1, wd);
    mn0 = block_ext<true>(mn0, we);
    mn1 = block_ext<true>(mn1, we);
    mx0 = block_ext<false>(mx0, we);
    mx1 = block_ext<false>(mx1, we);
    if (threadIdx.x != 0) return;
    out->n_nan = n_nan;
    out->n_bad_index = n_bad;
    write_class(out->cls[0], n0, s0, mn0, mx0);
    write_class(out->cls[1], n1, s1, mn1, mx1);
    // "all": the class that is not empty, bit for bit (either when both are), else the two merged, class 0 first
    if (!n1) write_class(out->cls[2], n0, s0, mn0, mx0);
    else if (!n0) write_class(out->cls[2], n1, s1, mn1, mx1);
    else write_class(out->cls[2], n0 + n1, s0 + s1, ext_best<true>(mn0, mn1), ext_best<false>(mx0, mx1));
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void analyze_pass2_kernel(const AnArgs g, const xvec_analyze_stats* stats, Part2* parts) {
    __shared__ double wd[kWaves];
    const double mean0 = stats->cls[0].mean, mean1 = stats->cls[1].mean;
    double q0 = 0.0, q1 = 0.0;
    const int64_t t0 = first_tile(blockIdx.x, g.tiles, g.blocks), t1 = first_tile(blockIdx.x + 1, g.tiles, g.blocks);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t base = tile * kTile + threadIdx.x;
        Trial tr[kItems];
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int64_t t = base + j * kThreads;
            if (t < g.trials.n) tr[j] = take_trial<ALL_PAIRS>(g, t); else tr[j].what = kSkip;
        }
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if (tr[j].what != kUse) continue;
            if (tr[j].target) {
                const double d = tr[j].score - mean1;
                q1 += d * d;
            } else {
                const double d = tr[j].score - mean0;
                q0 += d * d;
            }
        }
    }
    Part2 p;
    p.m2[0] = block_sum(q0, wd);
    p.m2[1] = block_sum(q1, wd);
    if (threadIdx.x == 0) parts[blockIdx.x] = p;
}

__global__ __launch_bounds__(kThreads) void analyze_merge2_kernel(const Part2* parts, int blocks, xvec_analyze_stats* out) {
    __shared__ double wd[kWaves];
    double q[2] = {0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        q[0] += parts[b].m2[0];
        q[1] += parts[b].m2[1];
    }
    q[0] = block_sum(q[0], wd);
    q[1] = block_sum(q[1], wd);
    if (threadIdx.x != 0) return;
    const long long n0 = out->cls[0].n, n1 = out->cls[1].n;
    if (n0) out->cls[0].var = q[0] / (double)n0;
    if (n1) out->cls[1].var = q[1] / (double)n1;
    if (!n1) {
        out->cls[2].var = out->cls[0].var;
    } else if (!n0) {
        out->cls[2].var = out->cls[1].var;
    } else {
        const double m = out->cls[2].mean, d0 = out->cls[0].mean - m, d1 = out->cls[1].mean - m;
        out->cls[2].var = ((q[0] + q[1]) + ((double)n0 * (d0 * d0) + (double)n1 * (d1 * d1))) / (double)(n0 + n1);
    }
}

// ================================================================ hardest

struct SelState {
    uint64_t prefix[2];                    // the digits chosen so far, in K space (below)
    uint32_t k_eff[2];                     // min(k, the class's trials)
    uint32_t k_rem[2];                     // the rank still looked for inside the prefix
    uint32_t above[2];                     // trials above the prefix
    uint32_t bucket[2];                    // trials in it
    uint32_t passes[2];                    // digits chosen
    uint32_t done[2];                      // bucket and above fit the candidates, or the key is complete
    uint32_t keep[2];                      // trials of the bucket that go into the candidates (the first by t)
    unsigned long long n_nan, n_bad;
};
static_assert(sizeof(SelState) <= kStateBytes, "analyze_plan.h: kStateBytes");
static_assert(sizeof(xvec_analyze_record) == kRecordBytes, "analyze_plan.h: kRecordBytes");

struct SelArgs {
    AnArgs a;
    uint32_t* hist;                        // [kPasses][2][kRadix]
    SelState* state;
    uint32_t *counts, *offsets;            // [4][kMaxBlocks]
    xvec_analyze_record* cand[2];
    int32_t k, cap;
};

// K space: the larger, the harder.  Class 0 (the highest non-target scores): the key; class 1 (the lowest target scores): its complement.
__device__ __forceinline__ uint64_t hard_key(double s, bool target) {
    const uint64_t k = snorm_keys::key_of(s);
    return target ? ~k : k;
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void analyze_digit_kernel(const SelArgs g, int pass) {
    __shared__ uint32_t h[2 * kRadix];
    __shared__ uint32_t cnt[2];
    const SelState st = *g.state;          // written by the walk of the pass before
    if (pass > 0 && st.done[0] && st.done[1]) return;
    for (int i = threadIdx.x; i < 2 * kRadix; i += kThreads) h[i] = 0;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n_nan = 0, n_bad = 0;
    const int64_t t0 = first_tile(blockIdx.x, g.a.tiles, g.a.blocks), t1 = first_tile(blockIdx.x + 1, g.a.tiles, g.a.blocks);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t base = tile * kTile + threadIdx.x;
        Trial tr[kItems];
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int64_t t = base + j * kThreads;
            if (t < g.a.trials.n) tr[j] = take_trial<ALL_PAIRS>(g.a, t); else tr[j].what = kSkip;
        }
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            n_nan += tr[j].what == kNan;
            n_bad += tr[j].what == kBad;
            if (tr[j].what != kUse) continue;
            const int c = tr[j].target ? 1 : 0;
            if (pass > 0 && sel(st.done, c)) continue;
            const uint64_t K = hard_key(tr[j].score, tr[j].target);
            if (snorm_keys::in_prefix(K, sel(st.prefix, c), pass)) atomicAdd(&h[c * kRadix + snorm_keys::digit_of(K, pass)], 1u);
        }
    }
    if (pass == 0) {
        if (n_nan) atomicAdd(&cnt[0], n_nan);
        if (n_bad) atomicAdd(&cnt[1], n_bad);
    }
    __syncthreads();
    uint32_t* out = g.hist + (size_t)pass * 2 * kRadix;
    for (int i = threadIdx.x; i < 2 * kRadix; i += kThreads)
        if (h[i]) atomicAdd(&out[i], h[i]);
    if (pass == 0 && threadIdx.x == 0) {
        if (cnt[0]) atomicAdd(&g.state->n_nan, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&g.state->n_bad, (unsigned long long)cnt[1]);
    }
}

// The digit of `h` (one class's histogram of a pass) that holds the k_rem-th largest; thread 0 of a block calls it.
__device__ __forceinline__ void walk_step(const uint32_t* h, uint64_t& prefix, uint32_t& k_rem, uint32_t& above, uint32_t& bucket) {
    uint32_t over = 0;
    for (int d = kRadix - 1; d >= 0; --d) {
        const uint32_t c = h[d];
        if (snorm_keys::digit_holds_kth(over, c, k_rem)) {
            prefix = (prefix << snorm_keys::kDigitBits) | (uint32_t)d;
            k_rem -= over;
            above += over;
            bucket = c;
            return;
        }
        over += c;
    }
}

__global__ __launch_bounds__(kThreads) void analyze_walk_kernel(const SelArgs g, int pass) {
    __shared__ uint32_t h[2 * kRadix];
    __shared__ uint32_t wtot[kWaves];
    const uint32_t* in = g.hist + (size_t)pass * 2 * kRadix;
    for (int i = threadIdx.x; i < 2 * kRadix; i += kThreads) h[i] = in[i];
    __syncthreads();
    uint32_t n_class[2] = {0, 0};
    if (pass == 0) {
        n_class[0] = block_scan_array(h, (uint32_t*)nullptr, kRadix, wtot);
        n_class[1] = block_scan_array(h + kRadix, (uint32_t*)nullptr, kRadix, wtot);
    }
    if (threadIdx.x != 0) return;
    SelState st = *g.state;
    for (int c = 0; c < 2; ++c) {
        if (pass == 0) {
            st.k_eff[c] = st.k_rem[c] = n_class[c] < (uint32_t)g.k ? n_class[c] : (uint32_t)g.k;
            st.done[c] = st.k_eff[c] == 0;
        }
        if (st.done[c]) continue;
        walk_step(h + c * kRadix, st.prefix[c], st.k_rem[c], st.above[c], st.bucket[c]);
        st.passes[c] = (uint32_t)pass + 1;
        st.done[c] = (uint64_t)st.above[c] + st.bucket[c] <= (uint64_t)g.cap || pass == kPasses - 1;
    }
    *g.state = st;
}

// 1: above the class's prefix, 2: in it, 0: neither (or the class has nothing to give)
__device__ __forceinline__ uint32_t place_of(uint64_t K, const SelState& st, int c) {
    if (sel(st.k_eff, c) == 0) return 0;
    const int p = (int)sel(st.passes, c);
    const uint64_t hi = p == kPasses ? K : K >> shift_after(p), prefix = sel(st.prefix, c);
    return hi > prefix ? 1u : hi == prefix ? 2u : 0u;
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void analyze_count_kernel(const SelArgs g) {
    __shared__ uint32_t cnt[4];
    const SelState st = *g.state;
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n[4] = {0, 0, 0, 0};
    const int64_t t0 = first_tile(blockIdx.x, g.a.tiles, g.a.blocks), t1 = first_tile(blockIdx.x + 1, g.a.tiles, g.a.blocks);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t base = tile * kTile + threadIdx.x;
        Trial tr[kItems];
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int64_t t = base + j * kThreads;
            if (t < g.a.trials.n) tr[j] = take_trial<ALL_PAIRS>(g.a, t); else tr[j].what = kSkip;
        }
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if (tr[j].what != kUse) continue;
            const int c = tr[j].target ? 1 : 0;
            const uint32_t where = place_of(hard_key(tr[j].score, tr[j].target), st, c);
            n[0] += c == 0 && where == 1;
            n[1] += c == 0 && where == 2;
            n[2] += c == 1 && where == 1;
            n[3] += c == 1 && where == 2;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (n[i]) atomicAdd(&cnt[i], n[i]);
    __syncthreads();
    if (threadIdx.x < 4) g.counts[threadIdx.x * kMaxBlocks + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void analyze_offsets_kernel(const SelArgs g) {
    __shared__ uint32_t wtot[kWaves];
    uint32_t total[4];
    for (int i = 0; i < 4; ++i)
        total[i] = block_scan_array(g.counts + i * kMaxBlocks, g.offsets + i * kMaxBlocks, g.a.blocks, wtot);
    if (threadIdx.x != 0) return;
    for (int c = 0; c < 2; ++c) {
        const uint32_t room = (uint32_t)g.cap - g.state->above[c];      // above < k <= cap
        g.state->keep[c] = total[2 * c + 1] < room ? total[2 * c + 1] : room;
    }
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void analyze_write_kernel(const SelArgs g) {
    __shared__ uint64_t wtot[kWaves];
    const SelState st = *g.state;
    uint32_t at[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) at[i] = g.offsets[i * kMaxBlocks + blockIdx.x];
    const int64_t t0 = first_tile(blockIdx.x, g.a.tiles, g.a.blocks), t1 = first_tile(blockIdx.x + 1, g.a.tiles, g.a.blocks);
    for (int64_t tile = t0; tile < t1; ++tile) {
        for (int j = 0; j < kItems; ++j) {                         // slabs of kThreads trials in trial order
            const int64_t t = tile * kTile + j * kThreads + threadIdx.x;
            Trial tr{};
            tr.what = kSkip;
            if (t < g.a.trials.n) tr = take_trial<ALL_PAIRS>(g.a, t);
            const int c = tr.target ? 1 : 0;
            const uint32_t where = tr.what == kUse ? place_of(hard_key(tr.score, tr.target), st, c) : 0u;
            const int field = where ? 2 * c + (int)where - 1 : 0;
            const uint64_t packed = where ? (uint64_t)1 << (16 * field) : 0;
            if (!__syncthreads_or(where != 0)) continue;            // the same for every thread
            uint64_t total;
            const uint64_t before = block_excl_scan64(packed, wtot, &total);
            if (where) {
                const uint32_t rank = at[field] + (uint32_t)((before >> (16 * field)) & 0xffffu);
                const bool fits = where == 1 ? rank < (uint32_t)g.cap : rank < sel(st.keep, c);
                const uint32_t slot = where == 1 ? rank : sel(st.above, c) + rank;
                if (fits && slot < (uint32_t)g.cap) {
                    xvec_analyze_record r;
                    r.score = tr.score;
                    r.row = (int32_t)tr.row;
                    r.col = (int32_t)tr.col;
                    r.t = t;
                    sel(g.cand, c)[slot] = r;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) at[i] += (uint32_t)((total >> (16 * i)) & 0xffffu);
        }
    }
}

// descending K, then ascending place in the candidate buffer (which is ascending t)
__device__ __forceinline__ bool goes_first(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka > kb || (ka == kb && ia < ib);
}

__global__ __launch_bounds__(kThreads) void analyze_final_kernel(const SelArgs g, xvec_analyze_record* out0, xvec_analyze_record* out1,
                                                                 long long* counts) {
    __shared__ uint64_t skey[kMaxK];
    __shared__ uint32_t sidx[kMaxK];
    __shared__ uint32_t h[kRadix];
    __shared__ uint32_t wtot[kWaves];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_rem;
    const int c = blockIdx.x;
    const SelState st = *g.state;
    const xvec_analyze_record* cand = sel(g.cand, c);
    xvec_analyze_record* out = c ? out1 : out0;
    const uint32_t k_eff = sel(st.k_eff, c), above = sel(st.above, c), n_cand = above + sel(st.keep, c);
    if (threadIdx.x == 0) {
        counts[c] = k_eff;
        if (c == 0) {
            counts[2] = (long long)st.n_nan;
            counts[3] = (long long)st.n_bad;
        }
        s_prefix = sel(st.prefix, c);
        s_rem = sel(st.k_rem, c);
    }
    if (k_eff == 0) return;                                        // the same for every thread
    // the rest of the walk, over the bucket's part of the candidates
    for (int pass = (int)sel(st.passes, c); pass < kPasses; ++pass) {
        for (int i = threadIdx.x; i < kRadix; i += kThreads) h[i] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix;
        for (uint32_t i = above + threadIdx.x; i < n_cand; i += kThreads) {
            const uint64_t K = hard_key(cand[i].score, c != 0);
            if (snorm_keys::in_prefix(K, prefix, pass)) atomicAdd(&h[snorm_keys::digit_of(K, pass)], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t p = prefix;
            uint32_t rem = s_rem, more = 0, bucket = 0;
            walk_step(h, p, rem, more, bucket);
            s_prefix = p;
            s_rem = rem;
        }
        __syncthreads();
    }
    __syncthreads();
    const uint64_t kth = s_prefix;                                 // the whole key of the k-th hardest
    const uint32_t rem = s_rem;                                    // and how many of its equals belong to the list: the first by t
    for (int i = threadIdx.x; i < kMaxK; i += kThreads) {
        skey[i] = 0;                                               // below every key of a value: pads sort last
        sidx[i] = 0xffffffffu;
    }
    uint32_t sure_before = 0, equal_before = 0;
    for (uint32_t c0 = 0; c0 < n_cand; c0 += kThreads) {
        const uint32_t i = c0 + threadIdx.x;
        uint64_t K = 0;
        uint32_t sure = 0, equal = 0;
        if (i < n_cand) {
            K = hard_key(cand[i].score, c != 0);
            sure = i < above || K > kth;
            equal = !sure && K == kth;
        }
        uint32_t total;
        const uint32_t before = block_excl_scan(sure | (equal << 16), wtot, &total);
        const uint32_t eq_rank = equal_before + (before >> 16);
        if (sure || (equal && eq_rank < rem)) {
            const uint32_t eq_taken = eq_rank < rem ? eq_rank : rem;
            const uint32_t pos = sure_before + (before & 0xffffu) + eq_taken;
            if (pos < (uint32_t)kMaxK) {
                skey[pos] = K;
                sidx[pos] = i;
            }
        }
        sure_before += total & 0xffffu;
        equal_before += total >> 16;
    }
    __syncthreads();
    // bitonic sort of the kMaxK slots
    for (uint32_t size = 2; size <= (uint32_t)kMaxK; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < (uint32_t)kMaxK / 2; i += kThreads) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;                  // this run puts the first-going at the low index
                const uint64_t ka = skey[lo], kb = skey[hi];
                const uint32_t ia = sidx[lo], ib = sidx[hi];
                if (goes_first(kb, ib, ka, ia) == up) {
                    skey[lo] = kb, skey[hi] = ka;
                    sidx[lo] = ib, sidx[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t j = threadIdx.x; j < k_eff; j += kThreads) {
        const uint32_t i = sidx[j];
        if (i < n_cand) out[j] = cand[i];                          // (a pad never gets here: the survivors are k_eff)
    }
}

// ================================================================ host

thread_local ErrorChannel g_aerr;

int refused(const Refusal& why, bool too_large = false) {
    return g_aerr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why);
}

AnArgs an_args(const TrialArgs& trials, bool upper_only) {
    AnArgs a{};
    a.trials = trials;
    a.upper_only = upper_only;
    a.tiles = tiles_of(trials.n);
    a.blocks = blocks_of(trials.n);
    return a;
}

int run_summary(const TrialArgs& trials, bool all_pairs, bool upper_only, const xvec_analyze_bins* bins, xvec_analyze_stats* out,
                int64_t* counts, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const SummaryLayout l = summary_layout(trials.n, bins ? bins->n_bins : 0);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_aerr))) return rc;
    const AnArgs a = an_args(trials, upper_only);
    Part1* p1 = part<Part1>(workspace, l.part1);
    Part2* p2 = part<Part2>(workspace, l.part2);
    HistArgs h{};
    const unsigned grid = (unsigned)l.blocks;
    if (bins) {
        h.width = bins->width;
        h.first = bins->first;
        h.n_bins = bins->n_bins;
        h.rounding = bins->rounding;
        h.copies = copies_of(bins->n_bins, bins->hist_copies);
        h.counts = reinterpret_cast<unsigned long long*>(counts);
        const hipError_t e = hipMemsetAsync(counts, 0, (size_t)slots_of(bins->n_bins) * sizeof(int64_t), s);
        if (e != hipSuccess) return g_aerr.fail(XVEC_ERR_HIP, "clearing the histogram failed: %s", hipGetErrorString(e));
        if (all_pairs) analyze_pass1_kernel<true, true><<<grid, kThreads, 0, s>>>(a, h, p1);
        else analyze_pass1_kernel<false, true><<<grid, kThreads, 0, s>>>(a, h, p1);
    } else {
        if (all_pairs) analyze_pass1_kernel<true, false><<<grid, kThreads, 0, s>>>(a, h, p1);
        else analyze_pass1_kernel<false, false><<<grid, kThreads, 0, s>>>(a, h, p1);
    }
    if ((rc = g_aerr.launch_ok("analyze_pass1_kernel"))) return rc;
    analyze_merge1_kernel<<<1, kThreads, 0, s>>>(p1, (int)l.blocks, out);
    if ((rc = g_aerr.launch_ok("analyze_merge1_kernel"))) return rc;
    if (all_pairs) analyze_pass2_kernel<true><<<grid, kThreads, 0, s>>>(a, out, p2);
    else analyze_pass2_kernel<false><<<grid, kThreads, 0, s>>>(a, out, p2);
    if ((rc = g_aerr.launch_ok("analyze_pass2_kernel"))) return rc;
    analyze_merge2_kernel<<<1, kThreads, 0, s>>>(p2, (int)l.blocks, out);
    return g_aerr.launch_ok("analyze_merge2_kernel");
}

int run_hardest(const TrialArgs& trials, bool all_pairs, bool upper_only, const xvec_analyze_select* sel,
                xvec_analyze_record* out0, xvec_analyze_record* out1, int64_t* counts, void* workspace, size_t workspace_bytes,
                hipStream_t s) {
    const HardestLayout l = hardest_layout(trials.n, sel->k, sel->cand_cap);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_aerr))) return rc;
    SelArgs g{};
    g.a = an_args(trials, upper_only);
    g.hist = part<uint32_t>(workspace, l.hist);
    g.state = part<SelState>(workspace, l.state);
    g.counts = part<uint32_t>(workspace, l.counts);
    g.offsets = part<uint32_t>(workspace, l.offsets);
    g.cand[0] = part<xvec_analyze_record>(workspace, l.cand[0]);
    g.cand[1] = part<xvec_analyze_record>(workspace, l.cand[1]);
    g.k = sel->k;
    g.cap = l.cap;
    // the digit tables and the state behind them, in one piece
    const hipError_t e = hipMemsetAsync(g.hist, 0, l.state - l.hist + kStateBytes, s);
    if (e != hipSuccess) return g_aerr.fail(XVEC_ERR_HIP, "clearing the digit tables failed: %s", hipGetErrorString(e));
    const unsigned grid = (unsigned)l.blocks;
    for (int pass = 0; pass < kPasses; ++pass) {
        if (all_pairs) analyze_digit_kernel<true><<<grid, kThreads, 0, s>>>(g, pass);
        else analyze_digit_kernel<false><<<grid, kThreads, 0, s>>>(g, pass);
        if ((rc = g_aerr.launch_ok("analyze_digit_kernel"))) return rc;
        analyze_walk_kernel<<<1, kThreads, 0, s>>>(g, pass);
        if ((rc = g_aerr.launch_ok("analyze_walk_kernel"))) return rc;
    }
    if (all_pairs) analyze_count_kernel<true><<<grid, kThreads, 0, s>>>(g);
    else analyze_count_kernel<false><<<grid, kThreads, 0, s>>>(g);
    if ((rc = g_aerr.launch_ok("analyze_count_kernel"))) return rc;
    analyze_offsets_kernel<<<1, kThreads, 0, s>>>(g);
    if ((rc = g_aerr.launch_ok("analyze_offsets_kernel"))) return rc;
    if (all_pairs) analyze_write_kernel<true><<<grid, kThreads, 0, s>>>(g);
    else analyze_write_kernel<false><<<grid, kThreads, 0, s>>>(g);
    if ((rc = g_aerr.launch_ok("analyze_write_kernel"))) return rc;
    analyze_final_kernel<<<2, kThreads, 0, s>>>(g, out0, out1, reinterpret_cast<long long*>(counts));
    return g_aerr.launch_ok("analyze_final_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_analyze_last_error(void) { return g_aerr.c_str(); }

int xvec_analyze_plan_host(int64_t n_trials, int32_t n_bins, int64_t* out) {
    Refusal why;
    if (check_plan_query(n_trials, n_bins, out, why)) return refused(why);
    out[0] = tiles_of(n_trials);
    out[1] = blocks_of(n_trials);
    out[2] = most_tiles(n_trials);
    out[3] = sum_depth(n_trials);
    out[4] = n_bins ? max_copies(n_bins) : 0;
    out[5] = out[4];
    out[6] = kDefaultCand;
    out[7] = kSecondTileFrom;
    return XVEC_OK;
}

size_t xvec_analyze_summary_workspace_bytes(int64_t n_trials, int32_t n_bins) { return summary_layout(n_trials, n_bins).total; }

size_t xvec_analyze_hardest_workspace_bytes(int64_t n_trials, int32_t k, int32_t cand_cap) {
    return hardest_layout(n_trials, k, cand_cap).total;
}

int xvec_analyze_summary(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                         const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, const xvec_analyze_bins* bins,
                         xvec_analyze_stats* out, int64_t* counts, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large);
    if (check_bins(bins, counts, why) || check_stats(out, why)) return refused(why);
    return run_summary(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, false, bins, out,
                       counts, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int xvec_analyze_summary_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                                   const int32_t* col_class, int32_t skip_diagonal, int32_t upper_only,
                                   const xvec_analyze_bins* bins, xvec_analyze_stats* out, int64_t* counts, void* workspace,
                                   size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_all_pairs(scores, ld, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large);
    if (check_bins(bins, counts, why) || check_stats(out, why)) return refused(why);
    return run_summary(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true,
                       upper_only != 0, bins, out, counts, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int xvec_analyze_hardest(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                         const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, const xvec_analyze_select* select,
                         xvec_analyze_record* nontarget_out, xvec_analyze_record* target_out, int64_t* counts, void* workspace,
                         size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large);
    if (check_select(select, why) || check_lists(nontarget_out, target_out, counts, why)) return refused(why);
    return run_hardest(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, false, select,
                       nontarget_out, target_out, counts, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int xvec_analyze_hardest_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                                   const int32_t* col_class, int32_t skip_diagonal, int32_t upper_only,
                                   const xvec_analyze_select* select, xvec_analyze_record* nontarget_out,
                                   xvec_analyze_record* target_out, int64_t* counts, void* workspace, size_t workspace_bytes,
                                   xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_all_pairs(scores, ld, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large);
    if (check_select(select, why) || check_lists(nontarget_out, target_out, counts, why)) return refused(why);
    return run_hardest(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true,
                       upper_only != 0, select, nontarget_out, target_out, counts, workspace, workspace_bytes,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
