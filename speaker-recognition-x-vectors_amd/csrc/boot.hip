// The bootstrap of trial evaluation: EER and minDCF of n_boot resamples of the groups (speakers) of a trial list.
// C ABI, the weights and the definitions: include/xvec_boot.h.  Plan, checks and the two maps: boot_plan.h.  The score key,
// the trial reader, the block primitives and the candidate records: trial_device.h; the sort: trial_sort.h, here with a 32-bit
// payload (this translation unit compiles that instantiation, and with it sorted_order of xvec_eval_sorted_order).
// A resample changes the weight of a trial, not its place, so the pairs are sorted ONCE; a replicate is a weighted prefix sum
// and sweep over that order.  Stages:
//   gather + key   as eval.hip, with the payload of the mode: the packed group ids and the bit, or the index and the bit
//   sort           trial_sort.h
//   per batch of replicates (boot_plan.h: batch_size):
//     counts       per (replicate, side): G draws into an LDS table of packed 16-bit counts (integer atomics), written as uint16
//     tile sums    per (tile, chunk of replicates): the tile's payloads are loaded once, the chunk's replicates loop over them
//     scan         per replicate: the 64-bit scan over the tiles, and the totals P_b, P_b + N_b
//     sweep        per (tile, chunk): the weights again, the in-tile 64-bit scan, the candidates of eval.hip
//     final        per replicate: one block reduces the tiles' candidates and writes the record
//   summary        the counters
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "../../include/xvec_boot.h"
#include "../../include/xvec_hip.h"
#include "boot_plan.h"
#include "host_support.h"
#include "trial_device.h"
#include "trial_plan.h"
#include "trial_sort.h"

namespace xvec {
namespace {

using namespace trial_device;
using namespace boot_plan;
using trial_sort::kWaves;
using trial_sort::SortBufs;

static_assert(kThreads == trial_sort::kThreads && kItems == trial_sort::kItems && kRadix == trial_sort::kRadix, "one tile");
static_assert(sizeof(EerCand) == 24 && sizeof(DcfCand) == 24 && kPartialBytes == 72, "boot_plan.h: the partials of a tile");

// counters in the workspace (uint64 each)
enum { kCntNan = 0, kCntBad = 1, kCntSkipped = 2, kCntBadGroup = 3, kCntDegenerate = 4, kCntOverflow = 5 };
constexpr int kWhatBadGroup = 4;              // beside trial_device's kUse .. kSkip

enum { kModeOrder = 0, kModeGroups = 1, kModePoisson = 2 };

struct BootArgs {
    TrialArgs trials;
    const int32_t *row_group, *col_group;
    int32_t g_rows, g_cols, joint, n_boot;
    uint64_t seed;
    double c_miss, c_fa, p_target;
    uint32_t *keys, *pay;
    unsigned long long* counters;
    uint16_t* tables;                         // [batch, g_rows + g_cols]
    uint64_t *sums, *totals;
    EerCand* eer;
    DcfCand* dcf;
    uint64_t* below;                          // [batch, tiles]: weighted trials at or below the tile's EER candidate
    int64_t tiles;
    int32_t b0, batch;                        // the batch holds the records b0 .. b0 + batch - 1 (those up to n_boot)
};

// ---------------------------------------------------------------- gather and key

template <bool ALL_PAIRS, int MODE>
__global__ __launch_bounds__(kThreads) void boot_gather_kernel(const BootArgs g) {
    __shared__ uint32_t cnt[4];
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t n_nan = 0, n_bad = 0, n_skip = 0, n_group = 0;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t t = base + k * kThreads + threadIdx.x;
        if (t >= g.trials.n) break;
        const Trial tr = locate_trial<ALL_PAIRS>(g.trials, t);
        int what = tr.what;
        uint32_t gr = 0, gc = 0;
        if (MODE == kModeGroups && what == kUse) {
            if (g.row_group) {
                const int32_t x = g.row_group[tr.row];
                if (x < 0 || x >= g.g_rows) what = kWhatBadGroup; else gr = (uint32_t)x;
            }
            if (g.col_group && what == kUse) {
                const int32_t x = g.col_group[tr.col];
                if (x < 0 || x >= g.g_cols) what = kWhatBadGroup; else gc = (uint32_t)x;
            }
        }
        double score = 0.0;
        if (what == kUse) {
            score = g.trials.scores[tr.row * g.trials.ld + tr.col];
            if (score != score) what = kNan;
        }
        const uint32_t bit = what == kUse ? (tr.target ? 1u : 0u) : (uint32_t)kBitVoid;
        n_nan += what == kNan;
        n_bad += what == kBad;
        n_skip += what == kSkip;
        n_group += what == kWhatBadGroup;
        g.keys[t] = what == kUse ? score_key(score) : kKeyVoid;
        g.pay[t] = MODE == kModeOrder ? (uint32_t)t : MODE == kModeGroups ? pack_groups(gr, gc, bit) : pack_index((uint32_t)t, bit & 1u);
    }
    if (n_nan) atomicAdd(&cnt[kCntNan], n_nan);
    if (n_bad) atomicAdd(&cnt[kCntBad], n_bad);
    if (n_skip) atomicAdd(&cnt[kCntSkipped], n_skip);
    if (n_group) atomicAdd(&cnt[kCntBadGroup], n_group);
    __syncthreads();
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&g.counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

__device__ __forceinline__ int64_t kept(const BootArgs& g) {      // the sorted prefix: the trials that count
    return g.trials.n - (int64_t)(g.counters[kCntNan] + g.counters[kCntBad] + g.counters[kCntSkipped] + g.counters[kCntBadGroup]);
}

// ---------------------------------------------------------------- counts: block (replicate of the batch, side)

__global__ __launch_bounds__(kThreads) void boot_counts_kernel(const BootArgs g) {
    __shared__ uint32_t h[kMaxGroups / 2];     // two 16-bit counts per word: a count is at most G <= 16384, no carry crosses
    const int side = blockIdx.y;
    const int32_t b = g.b0 + (int32_t)blockIdx.x;
    const uint32_t G = side == 0 ? (uint32_t)g.g_rows : (uint32_t)g.g_cols;
    if (b < 1 || b > g.n_boot || G == 0 || (side == 1 && g.joint)) return;      // the same for every thread of the block
    for (uint32_t i = threadIdx.x; i < (G + 1) / 2; i += kThreads) h[i] = 0;
    __syncthreads();
    for (uint32_t quad = threadIdx.x; quad * 4 < G; quad += kThreads) {
        const philox::Words w = draw_words(quad, (uint32_t)b, (uint32_t)side, g.seed);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (quad * 4 + q < G) {
                const uint32_t grp = pick_group(w.w[q], G);
                atomicAdd(&h[grp >> 1], 1u << (16 * (grp & 1u)));
            }
        }
    }
    __syncthreads();
    uint16_t* out = g.tables + (size_t)blockIdx.x * (size_t)(g.g_rows + g.g_cols) + (side ? g.g_rows : 0);
    for (uint32_t i = threadIdx.x; i < G; i += kThreads) out[i] = (uint16_t)(h[i >> 1] >> (16 * (i & 1u)));
}

// ---------------------------------------------------------------- the weight of a sorted trial

struct Tables {
    const uint16_t *rows, *cols;              // the replicate's count tables; null: the factor 1
};

__device__ __forceinline__ Tables tables_of(const BootArgs& g, int rl) {
    const uint16_t* t = g.tables + (size_t)rl * (size_t)(g.g_rows + g.g_cols);
    Tables r;
    r.rows = g.row_group ? t : nullptr;
    r.cols = g.col_group ? (g.joint ? t : t + g.g_rows) : nullptr;
    return r;
}

// record 0 is the point estimate: every weight 1
template <bool POISSON>
__device__ __forceinline__ uint32_t weight_of(uint32_t pay, int32_t b, const Tables& tb, uint64_t seed) {
    if (b == 0) return 1u;
    if (POISSON) return trial_poisson(seed, (uint32_t)b, packed_index(pay));
    uint32_t w = 1u;
    if (tb.rows) w *= tb.rows[packed_row(pay)];
    if (tb.cols) w *= tb.cols[packed_col(pay)];
    return w;                                 // at most 2^14 * 2^14
}

template <bool POISSON>
__device__ __forceinline__ bool target_of(uint32_t pay) {
    return POISSON ? packed_index_bit(pay) == 1u : packed_bit(pay) == 1u;
}

// ---------------------------------------------------------------- tile sums: block (tile, chunk of replicates)

template <bool POISSON>
__global__ __launch_bounds__(kThreads) void boot_tile_sums_kernel(const BootArgs g) {
    __shared__ long long wsum[kWaves];
    const int64_t m = kept(g);
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t pay[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        pay[k] = i < m ? g.pay[i] : 0u;
    }
#pragma unroll 1
    for (int rr = 0; rr < kChunk; ++rr) {
        const int rl = (int)blockIdx.y * kChunk + rr;
        const int32_t b = g.b0 + rl;
        if (rl >= g.batch || b > g.n_boot) break;                 // the same for every thread of the block
        const Tables tb = tables_of(g, rl);
        long long st = 0, sa = 0;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            if (base + k * kThreads + threadIdx.x < m) {
                const uint32_t w = weight_of<POISSON>(pay[k], b, tb, g.seed);
                sa += w;
                if (target_of<POISSON>(pay[k])) st += w;
            }
        }
        const long long T = block_count(st, wsum), A = block_count(sa, wsum);
        if (threadIdx.x == 0) {
            uint64_t* out = g.sums + ((size_t)rl * (size_t)g.tiles + blockIdx.x) * 2;
            out[0] = (uint64_t)T;
            out[1] = (uint64_t)A;
        }
    }
}

// ---------------------------------------------------------------- scan over the tiles: one block per replicate

__global__ __launch_bounds__(kThreads) void boot_scan_kernel(const BootArgs g) {
    __shared__ uint64_t wtot[kWaves];
    const int rl = blockIdx.x;
    if (g.b0 + rl > g.n_boot) return;
    uint64_t* v = g.sums + (size_t)rl * (size_t)g.tiles * 2;
    uint64_t carry_t = 0, carry_a = 0;
    for (int64_t c0 = 0; c0 < g.tiles; c0 += kThreads) {
        const int64_t i = c0 + threadIdx.x;
        const uint64_t t = i < g.tiles ? v[2 * i] : 0ull, a = i < g.tiles ? v[2 * i + 1] : 0ull;
        uint64_t tot_t, tot_a;
        const uint64_t et = block_excl_scan64(t, wtot, &tot_t);
        const uint64_t ea = block_excl_scan64(a, wtot, &tot_a);
        if (i < g.tiles) {
            v[2 * i] = carry_t + et;
            v[2 * i + 1] = carry_a + ea;
        }
        carry_t += tot_t;
        carry_a += tot_a;
    }
    if (threadIdx.x == 0) {
        g.totals[2 * rl] = carry_t;           // P_b
        g.totals[2 * rl + 1] = carry_a;       // P_b + N_b
    }
}

// ---------------------------------------------------------------- sweep: block (tile, chunk of replicates)

template <bool POISSON>
__global__ __launch_bounds__(kThreads) void boot_sweep_kernel(const BootArgs g) {
    __shared__ uint64_t wtot[kWaves];
    __shared__ EerCand s_eer[kThreads];
    __shared__ DcfCand s_dcf[kThreads];
    const int64_t m = kept(g);
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    // what does not change from replicate to replicate, as masks over the thread's items: inside the sorted prefix, a target,
    // the last of a run of equal keys
    uint32_t pay[kItems], in_mask = 0, target_mask = 0, end_mask = 0;
    {
        uint32_t key[kItems + 1];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const bool in = base + k < m;
            key[k] = in ? g.keys[base + k] : 0u;
            pay[k] = in ? g.pay[base + k] : 0u;
            in_mask |= (uint32_t)in << k;
            target_mask |= (uint32_t)(in && target_of<POISSON>(pay[k])) << k;
        }
        key[kItems] = base + kItems < m ? g.keys[base + kItems] : 0u;
#pragma unroll
        for (int k = 0; k < kItems; ++k) end_mask |= (uint32_t)(base + k + 1 >= m || key[k + 1] != key[k]) << k;
        end_mask &= in_mask;
    }
#pragma unroll 1
    for (int rr = 0; rr < kChunk; ++rr) {
        const int rl = (int)blockIdx.y * kChunk + rr;
        const int32_t b = g.b0 + rl;
        if (rl >= g.batch || b > g.n_boot) break;                 // the same for every thread of the block
        const Tables tb = tables_of(g, rl);
        const int64_t P = (int64_t)g.totals[2 * rl], A = (int64_t)g.totals[2 * rl + 1], N = A - P;
        uint32_t w[kItems];
        uint64_t st = 0, sa = 0;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            w[k] = (in_mask >> k) & 1u ? weight_of<POISSON>(pay[k], b, tb, g.seed) : 0u;
            sa += w[k];
            if ((target_mask >> k) & 1u) st += w[k];
        }
        const uint64_t* off = g.sums + ((size_t)rl * (size_t)g.tiles + blockIdx.x) * 2;
        int64_t tp = (int64_t)(block_excl_scan64(st, wtot, nullptr) + off[0]);
        int64_t ta = (int64_t)(block_excl_scan64(sa, wtot, nullptr) + off[1]);
        EerCand be = no_eer_cand();
        DcfCand bd = no_dcf_cand();
        int64_t be_below = 0;                                         // weighted trials at or below this thread's EER candidate
        if (replicate_state(P, A) == 0) {
#pragma unroll
            for (int k = 0; k < kItems; ++k) {
                ta += w[k];
                if ((target_mask >> k) & 1u) tp += w[k];
                if (!((end_mask >> k) & 1u) || ta == 0) continue;    // inside a run of equal scores, or below every score of the resample
                const int64_t i = base + k;
                consider(i, tp, ta - tp, P, N, g.c_miss, g.c_fa, g.p_target, be, bd);
                if (be.idx == i) be_below = ta;
            }
        }
        const int64_t mine = be.idx;
        be = block_best(be, s_eer);
        bd = block_best(bd, s_dcf);
        if (mine == be.idx && (mine != kNoIdx || threadIdx.x == 0))       // the one thread that owns the winner (none: thread 0)
            g.below[(size_t)rl * (size_t)g.tiles + blockIdx.x] = (uint64_t)be_below;
        if (threadIdx.x == 0) {
            g.eer[(size_t)rl * (size_t)g.tiles + blockIdx.x] = be;
            g.dcf[(size_t)rl * (size_t)g.tiles + blockIdx.x] = bd;
        }
    }
}

// ---------------------------------------------------------------- final: one block per replicate

__global__ __launch_bounds__(kThreads) void boot_final_kernel(const BootArgs g, xvec_boot_record* records) {
    __shared__ EerCand s_eer[kThreads];
    __shared__ DcfCand s_dcf[kThreads];
    const int rl = blockIdx.x;
    const int32_t b = g.b0 + rl;
    if (b > g.n_boot) return;
    EerCand be = no_eer_cand();
    DcfCand bd = no_dcf_cand();
    for (int64_t t = threadIdx.x; t < g.tiles; t += kThreads) {
        const EerCand ce = g.eer[(size_t)rl * (size_t)g.tiles + t];
        const DcfCand cd = g.dcf[(size_t)rl * (size_t)g.tiles + t];
        if (better(ce, be)) be = ce;
        if (better(cd, bd)) bd = cd;
    }
    be = block_best(be, s_eer);
    bd = block_best(bd, s_dcf);
    if (threadIdx.x != 0) return;
    const int64_t m = kept(g);
    const int64_t P = (int64_t)g.totals[2 * rl], A = (int64_t)g.totals[2 * rl + 1], N = A - P;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    xvec_boot_record r;
    r.eer = r.eer_threshold = r.far = r.frr = r.min_dcf = r.min_dcf_threshold = nan;
    r.n_target = P;
    r.n_nontarget = N;
    const int state = replicate_state(P, A);
    if (b >= 1 && state == 1) atomicAdd(&g.counters[kCntDegenerate], 1ull);
    if (b >= 1 && state == 2) atomicAdd(&g.counters[kCntOverflow], 1ull);
    if (state == 0 && be.idx != kNoIdx && bd.idx != kNoIdx && be.idx < m && bd.idx < m) {
        const Rates at = rates_at(be.tp, (int64_t)g.below[(size_t)rl * (size_t)g.tiles + be.idx / kTile], P, N);
        r.far = at.far;
        r.frr = at.frr;
        r.eer = at.eer;
        r.eer_threshold = (double)key_score(g.keys[be.idx]);
        r.min_dcf = bd.val;
        r.min_dcf_threshold = (double)key_score(g.keys[bd.idx]);
    }
    records[b] = r;
}

__global__ void boot_summary_kernel(const unsigned long long* counters, xvec_boot_summary* out) {
    xvec_boot_summary s;
    s.n_nan = (int64_t)counters[kCntNan];
    s.n_bad_index = (int64_t)counters[kCntBad];
    s.n_bad_group = (int64_t)counters[kCntBadGroup];
    s.n_degenerate = (int64_t)counters[kCntDegenerate];
    s.n_overflow = (int64_t)counters[kCntOverflow];
    *out = s;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_berr;

int refused(const Refusal& why, bool too_large = false) {
    return g_berr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why);
}

template <int MODE>
int launch_gather(const BootArgs& g, bool all_pairs, hipStream_t s, ErrorChannel& err) {
    const unsigned grid = (unsigned)tiles_of(g.trials.n);
    if (all_pairs) boot_gather_kernel<true, MODE><<<grid, kThreads, 0, s>>>(g);
    else boot_gather_kernel<false, MODE><<<grid, kThreads, 0, s>>>(g);
    return err.launch_ok("boot_gather_kernel");
}

int clear_counters(unsigned long long* counters, hipStream_t s, ErrorChannel& err) {
    const hipError_t e = hipMemsetAsync(counters, 0, kCounters * sizeof(unsigned long long), s);
    return e == hipSuccess ? XVEC_OK : err.fail(XVEC_ERR_HIP, "clearing the counters failed: %s", hipGetErrorString(e));
}

template <bool POISSON>
int run_batch(const BootArgs& g, xvec_boot_record* records, hipStream_t s) {
    const dim3 grid((unsigned)g.tiles, (unsigned)(g.batch / kChunk));
    int rc;
    if (!POISSON) {
        boot_counts_kernel<<<dim3((unsigned)g.batch, 2), kThreads, 0, s>>>(g);
        if ((rc = g_berr.launch_ok("boot_counts_kernel"))) return rc;
    }
    boot_tile_sums_kernel<POISSON><<<grid, kThreads, 0, s>>>(g);
    if ((rc = g_berr.launch_ok("boot_tile_sums_kernel"))) return rc;
    boot_scan_kernel<<<(unsigned)g.batch, kThreads, 0, s>>>(g);
    if ((rc = g_berr.launch_ok("boot_scan_kernel"))) return rc;
    boot_sweep_kernel<POISSON><<<grid, kThreads, 0, s>>>(g);
    if ((rc = g_berr.launch_ok("boot_sweep_kernel"))) return rc;
    boot_final_kernel<<<(unsigned)g.batch, kThreads, 0, s>>>(g, records);
    return g_berr.launch_ok("boot_final_kernel");
}

int run(const TrialArgs& trials, bool all_pairs, const xvec_boot_params* p, xvec_boot_summary* summary, xvec_boot_record* records,
        void* workspace, size_t workspace_bytes, hipStream_t s) {
    const Layout l = make_layout(trials.n, p->n_boot, p->n_row_groups, p->n_col_groups);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_berr))) return rc;
    const bool poisson = !p->row_group && !p->col_group;
    BootArgs g{};
    g.trials = trials;
    g.row_group = p->row_group;
    g.col_group = p->col_group;
    g.g_rows = p->n_row_groups;
    g.g_cols = p->n_col_groups;
    g.joint = p->joint != 0;
    g.n_boot = p->n_boot;
    g.seed = p->seed;
    g.c_miss = p->c_miss;
    g.c_fa = p->c_fa;
    g.p_target = p->p_target;
    g.keys = part<uint32_t>(workspace, l.keys[0]);
    g.pay = part<uint32_t>(workspace, l.pay[0]);
    g.counters = part<unsigned long long>(workspace, l.counters);
    g.tables = part<uint16_t>(workspace, l.tables);
    g.sums = part<uint64_t>(workspace, l.sums);
    g.totals = part<uint64_t>(workspace, l.totals);
    g.eer = part<EerCand>(workspace, l.eer);
    g.dcf = part<DcfCand>(workspace, l.dcf);
    g.below = part<uint64_t>(workspace, l.below);
    g.tiles = l.tiles;
    g.batch = l.batch;
    if ((rc = clear_counters(g.counters, s, g_berr))) return rc;
    if ((rc = poisson ? launch_gather<kModePoisson>(g, all_pairs, s, g_berr) : launch_gather<kModeGroups>(g, all_pairs, s, g_berr)))
        return rc;
    const SortBufs<uint32_t> bufs{{g.keys, part<uint32_t>(workspace, l.keys[1])}, {g.pay, part<uint32_t>(workspace, l.pay[1])},
                                  part<uint32_t>(workspace, l.hist), part<uint32_t>(workspace, l.hist_sums)};
    if ((rc = trial_sort::sort_pairs(bufs, trials.n, s, g_berr))) return rc;
    for (int64_t b0 = 0; b0 <= p->n_boot; b0 += l.batch) {
        g.b0 = (int32_t)b0;
        if ((rc = poisson ? run_batch<true>(g, records, s) : run_batch<false>(g, records, s))) return rc;
    }
    boot_summary_kernel<<<1, 1, 0, s>>>(g.counters, summary);
    return g_berr.launch_ok("boot_summary_kernel");
}

// the workspace of sorted_order: the sort's buffers and the counters
struct OrderLayout {
    size_t keys[2], pay[2], hist, hist_sums, counters, total;
};

OrderLayout order_layout(int64_t n) {
    OrderLayout l{};
    const size_t hist_len = (size_t)tiles_of(n) * kRadix;
    Carver c;
    for (int i = 0; i < 2; ++i) l.keys[i] = c.take_bytes((size_t)n * 4);
    for (int i = 0; i < 2; ++i) l.pay[i] = c.take_bytes((size_t)n * 4);
    l.hist = c.take_bytes(hist_len * 4);
    l.hist_sums = c.take_bytes((size_t)tiles_of((int64_t)hist_len) * 4);
    l.counters = c.take_bytes(kCounters * 8);
    l.total = c.total();
    return l;
}

}  // namespace

namespace trial_sort {

size_t sorted_order_bytes(int64_t n) { return order_layout(n).total; }

int sorted_order(const trial_device::TrialArgs& trials, bool all_pairs, uint32_t* keys_out, uint32_t* order_out, void* workspace,
                 hipStream_t s, ErrorChannel& err) {
    const OrderLayout l = order_layout(trials.n);
    BootArgs g{};
    g.trials = trials;
    g.keys = part<uint32_t>(workspace, l.keys[0]);
    g.pay = part<uint32_t>(workspace, l.pay[0]);
    g.counters = part<unsigned long long>(workspace, l.counters);
    int rc;
    if ((rc = clear_counters(g.counters, s, err))) return rc;
    if ((rc = launch_gather<kModeOrder>(g, all_pairs, s, err))) return rc;
    const SortBufs<uint32_t> bufs{{g.keys, part<uint32_t>(workspace, l.keys[1])}, {g.pay, part<uint32_t>(workspace, l.pay[1])},
                                  part<uint32_t>(workspace, l.hist), part<uint32_t>(workspace, l.hist_sums)};
    if ((rc = sort_pairs(bufs, trials.n, s, err))) return rc;
    hipError_t e = hipMemcpyAsync(keys_out, g.keys, (size_t)trials.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(order_out, g.pay, (size_t)trials.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return err.fail(XVEC_ERR_HIP, "copying the sorted pairs failed: %s", hipGetErrorString(e));
    return XVEC_OK;
}

}  // namespace trial_sort
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_boot_last_error(void) { return g_berr.c_str(); }

size_t xvec_boot_workspace_bytes(int64_t n_trials, int32_t n_boot, int32_t n_row_groups, int32_t n_col_groups) {
    return make_layout(n_trials, n_boot, n_row_groups, n_col_groups).total;
}

int32_t xvec_boot_batch(int64_t n_trials, int32_t n_boot) { return batch_size(n_trials, n_boot); }
int32_t xvec_boot_batches(int64_t n_trials, int32_t n_boot) { return batch_count(n_trials, n_boot); }

int xvec_boot_trials(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                     const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, const xvec_boot_params* params,
                     xvec_boot_summary* summary, xvec_boot_record* records, void* workspace, size_t workspace_bytes,
                     xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large);
    if (check_params(params, why) || check_vector_groups(row_idx, params, why) || check_outputs(summary, records, why))
        return refused(why);
    return run(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, params, summary, records,
               workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int xvec_boot_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                        const int32_t* col_class, int32_t skip_diagonal, const xvec_boot_params* params,
                        xvec_boot_summary* summary, xvec_boot_record* records, void* workspace, size_t workspace_bytes,
                        xvec_stream stream) {
    Refusal why;
    bool too_large = false;
    if (trial_plan::check_all_pairs(scores, ld, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large);
    if (check_params(params, why) || check_outputs(summary, records, why)) return refused(why);
    return run(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true,
               params, summary, records, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int xvec_boot_counts_host(uint64_t seed, int32_t b, int32_t side, int32_t n_groups, uint16_t* counts_out) {
    Refusal why;
    if (check_host_counts(b, side, n_groups, counts_out, why)) return refused(why);
    for (int32_t i = 0; i < n_groups; ++i) counts_out[i] = 0;
    for (int32_t j = 0; j < n_groups; ++j)
        ++counts_out[drawn_group(seed, (uint32_t)b, (uint32_t)side, (uint32_t)j, (uint32_t)n_groups)];
    return XVEC_OK;
}

int xvec_boot_poisson_host(uint64_t seed, int32_t b, int64_t t, int32_t* weight_out) {
    Refusal why;
    if (check_host_poisson(b, t, weight_out, why)) return refused(why);
    *weight_out = (int32_t)trial_poisson(seed, (uint32_t)b, (uint32_t)t);
    return XVEC_OK;
}

}  // extern "C"
