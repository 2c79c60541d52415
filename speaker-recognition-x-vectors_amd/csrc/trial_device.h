// What the kernels of the trial family share: the score key of include/xvec_eval.h, the one reader that decides which trials
// count (eval.hip, calib.hip, report.hip: calibration and the DET curve are only right if all three leave out exactly the same
// trials), and the block primitives around it (snorm.hip takes its sum from here too).  After <hip/hip_runtime.h>.
//
// Every thread of the block must call a block primitive, and the result is in every thread.  The block is WAVES whole waves;
// WAVES is the size of the LDS array the caller hands in and MUST equal blockDim.x / 64 (256-thread blocks: 4, snorm's 512-thread
// blocks: 8): a smaller array is written past its end, a larger one read where no wave wrote.  Every unit declares its arrays as
// [kWaves] with kWaves = kThreads / 64 and launches these kernels with kThreads under __launch_bounds__(kThreads).  Each primitive
// syncs before it writes that array (the previous call's readers are done with it) and after, so calls may follow each other
// on one array.
#pragma once
#include <cstdint>

namespace xvec {
namespace trial_device {

// ---------------------------------------------------------------- the score key

constexpr uint8_t kBitVoid = 2;               // a trial left out (NaN, bad index, skipped diagonal): key kKeyVoid, sorts last
constexpr uint32_t kKeyVoid = 0xffffffffu;    // above the key of +inf (0xff800000); no finite score or infinity maps to it

// fp64 score -> fp32 (round to nearest even) -> key with key(a) < key(b) iff a < b; -0.0 and +0.0 share 0x80000000
__device__ __forceinline__ uint32_t score_key(double s) {
    uint32_t u = __float_as_uint(__double2float_rn(s));
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_score(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return __uint_as_float(u);
}

// ---------------------------------------------------------------- the trial forms

// A trial list (row_idx / col_idx / is_target; without index arrays trial t is cell (0, t)) or all pairs (every cell of the
// matrix a trial, a target where the classes of its row and column agree).
struct TrialArgs {
    const double* scores;
    int64_t ld, n_rows, n_cols, n;
    const int32_t* a;          // row_idx | row_class
    const int32_t* b;          // col_idx | col_class
    const uint8_t* is_target;  // trial list only
    int skip_diagonal;         // all pairs only
};

inline TrialArgs trial_args(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* a, const int32_t* b,
                            const uint8_t* is_target, int64_t n, bool skip_diagonal) {
    TrialArgs g{};
    g.scores = scores;
    g.ld = ld;
    g.n_rows = n_rows;
    g.n_cols = n_cols;
    g.n = n;
    g.a = a;
    g.b = b;
    g.is_target = is_target;
    g.skip_diagonal = skip_diagonal;
    return g;
}

enum { kUse = 0, kNan = 1, kBad = 2, kSkip = 3 };

struct Trial {
    int what;                  // kUse: it counts.  kNan: its score is NaN.  kBad: an index outside the matrix.  kSkip: a diagonal cell
    int64_t row, col;
    bool target;
    double score;              // read for kUse and kNan only: the cell of a bad index or a skipped one is never dereferenced
};

template <bool ALL_PAIRS>
__device__ __forceinline__ Trial read_trial(const TrialArgs& g, int64_t t) {
    Trial r;
    r.score = 0.0;
    if (ALL_PAIRS) {
        r.row = (int64_t)((uint32_t)t / (uint32_t)g.n_cols);       // t < 2^31, n_cols < 2^31
        r.col = t - r.row * g.n_cols;
        r.target = g.a[r.row] == g.b[r.col];
        r.what = g.skip_diagonal && r.row == r.col ? kSkip : kUse;
    } else {
        r.row = g.a ? (int64_t)g.a[t] : 0;
        r.col = g.b ? (int64_t)g.b[t] : t;
        r.target = g.is_target[t] != 0;
        r.what = r.row < 0 || r.row >= g.n_rows || r.col < 0 || r.col >= g.n_cols ? kBad : kUse;
    }
    if (r.what == kUse) {
        r.score = g.scores[r.row * g.ld + r.col];
        if (r.score != r.score) r.what = kNan;
    }
    return r;
}

// The index half of read_trial for a unit that reads several arrays per trial (fuse.hip): row, col, target and what (kUse, kBad
// or kSkip by the same tests); g.scores is not touched and score stays 0.  The caller reads its cells for kUse only.
template <bool ALL_PAIRS>
__device__ __forceinline__ Trial locate_trial(const TrialArgs& g, int64_t t) {
    Trial r;
    r.score = 0.0;
    if (ALL_PAIRS) {
        r.row = (int64_t)((uint32_t)t / (uint32_t)g.n_cols);
        r.col = t - r.row * g.n_cols;
        r.target = g.a[r.row] == g.b[r.col];
        r.what = g.skip_diagonal && r.row == r.col ? kSkip : kUse;
    } else {
        r.row = g.a ? (int64_t)g.a[t] : 0;
        r.col = g.b ? (int64_t)g.b[t] : t;
        r.target = g.is_target[t] != 0;
        r.what = r.row < 0 || r.row >= g.n_rows || r.col < 0 || r.col >= g.n_cols ? kBad : kUse;
    }
    return r;
}

// ---------------------------------------------------------------- block primitives

// Exclusive scan of one value per thread in thread order; *total (if given) receives the sum.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t (&wtot)[WAVES], uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    uint32_t add = 0, t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t s = wtot[w];
        if (w < wave) add += s;
        t += s;
    }
    if (total) *total = t;
    return add + x - v;
}

// The same in 64 bits (boot.hip: weighted counts do not fit 32).
template <int WAVES>
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t (&wtot)[WAVES], uint64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    uint64_t add = 0, t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint64_t s = wtot[w];
        if (w < wave) add += s;
        t += s;
    }
    if (total) *total = t;
    return add + x - v;
}

// One block walks in[0 .. n) in chunks of its thread count, in rising order, and returns the sum; out (if given, in itself
// or another array) receives the exclusive scan.
template <int WAVES>
__device__ __forceinline__ uint32_t block_scan_array(const uint32_t* in, uint32_t* out, int64_t n, uint32_t (&wtot)[WAVES]) {
    uint32_t carry = 0;
    for (int64_t c0 = 0; c0 < n; c0 += WAVES * 64) {
        const int64_t i = c0 + threadIdx.x;
        uint32_t total;
        const uint32_t e = block_excl_scan(i < n ? in[i] : 0u, wtot, &total);
        if (out && i < n) out[i] = carry + e;
        carry += total;
    }
    return carry;
}

// The combining order of the three reductions (include/xvec_calib.h, SUMMATION ORDER): a butterfly over the wave's lanes,
// offsets 1, 2, ..., 32 (every lane ends with the same bits: the partners of a step combine the same two numbers), then the
// waves' results in wave order.
template <typename T, int WAVES, typename F>
__device__ __forceinline__ T block_reduce(T v, T (&wbuf)[WAVES], F combine) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = combine(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wbuf[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = wbuf[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = combine(s, wbuf[w]);
    return s;
}

template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double (&wsum)[WAVES]) {
    return block_reduce(v, wsum, [](double a, double b) { return a + b; });
}

template <int WAVES>
__device__ __forceinline__ long long block_count(long long v, long long (&wsum)[WAVES]) {
    return block_reduce(v, wsum, [](long long a, long long b) { return a + b; });
}

// MIN: minimum, else maximum
template <bool MIN, int WAVES>
__device__ __forceinline__ double block_extreme(double v, double (&wbuf)[WAVES]) {
    return block_reduce(v, wbuf, [](double a, double b) { return MIN ? fmin(a, b) : fmax(a, b); });
}

// ---------------------------------------------------------------- candidate thresholds (eval.hip, boot.hip)

// A candidate threshold: objective, sorted index, targets at or below it.  Order: smaller objective, then smaller index --
// a total order, so the reduction gives the same winner whatever its shape.
struct EerCand {
    int64_t val, idx, tp;
};
struct DcfCand {
    double val;
    int64_t idx, tp;
};
__device__ __forceinline__ bool better(const EerCand& a, const EerCand& b) {
    return a.val < b.val || (a.val == b.val && a.idx < b.idx);
}
__device__ __forceinline__ bool better(const DcfCand& a, const DcfCand& b) {
    return a.val < b.val || (a.val == b.val && a.idx < b.idx);
}
constexpr int64_t kNoIdx = 0x7fffffffffffffffll;

__device__ __forceinline__ EerCand no_eer_cand() { return EerCand{kNoIdx, kNoIdx, 0}; }
__device__ __forceinline__ DcfCand no_dcf_cand() { return DcfCand{__longlong_as_double(0x7ff0000000000000ll), kNoIdx, 0}; }   // +inf

// The threshold at sorted index i with tp targets and nn non-targets at or below it, of P targets and N non-targets
// (P + N < 2^31: |fa P - tp N| < 2^62): both objectives of include/xvec_eval.h, kept where they beat be / bd.
__device__ __forceinline__ void consider(int64_t i, int64_t tp, int64_t nn, int64_t P, int64_t N, double c_miss, double c_fa,
                                         double p_target, EerCand& be, DcfCand& bd) {
    const int64_t fa = N - nn;                            // non-targets above the threshold
    const int64_t diff = fa * P - tp * N;
    const EerCand ce{diff < 0 ? -diff : diff, i, tp};
    if (better(ce, be)) be = ce;
    const double frr = (double)tp / (double)P, far = (double)fa / (double)N;
    const DcfCand cd{c_miss * frr * p_target + c_fa * far * (1.0 - p_target), i, tp};
    if (better(cd, bd)) bd = cd;
}

// What the winners say: far, frr, eer of the EER candidate at index be.idx, of which `below` trials lie at or below it.
struct Rates {
    double far, frr, eer;
};
__device__ __forceinline__ Rates rates_at(int64_t tp, int64_t below, int64_t P, int64_t N) {
    Rates r;
    const int64_t fa = N - (below - tp);
    r.far = (double)fa / (double)N;
    r.frr = (double)tp / (double)P;
    r.eer = (r.far + r.frr) / 2.0;
    return r;
}

// The best of one candidate per thread, in every thread; sh holds one per thread of the block.
template <typename C, int THREADS>
__device__ __forceinline__ C block_best(C mine, C (&sh)[THREADS]) {
    __syncthreads();
    sh[threadIdx.x] = mine;
    __syncthreads();
#pragma unroll
    for (int half = THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half && better(sh[threadIdx.x + half], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + half];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace trial_device
}  // namespace xvec
