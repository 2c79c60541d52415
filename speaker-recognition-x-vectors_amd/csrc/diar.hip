// Speaker diarization's clustering step: agglomerative clustering with average linkage of every recording's window scores.
// C ABI and the definitions: include/xvec_diar.h; the host-only half (checks, workspace layout, launch groups): diar_plan.h.
//   layout   one block: where each recording's working matrix starts (a prefix sum of mat_elems(n_r) over the recordings).
//   init     a wave per row of the batch: the row of the symmetric working copy from the upper triangle of S (the cells left
//            of the diagonal are the column above it), and the row's first best partner.
//   cluster  one block per recording, persistent over its merges.  Per live row the block keeps in LDS the best partner and
//            its score over the WHOLE row (the matrix is symmetric, so the lowest row that holds the largest score pairs with
//            a higher one: largest score, lowest i, lowest j), the cluster size, and per segment the cluster it is in.  A step:
//              1. block-wide argmax over the cached row bests, and the stop rule;
//              2. one pass over k that rewrites row i and column i, folds the new row's own best and compares every other
//                 row's cached best against its new cell; rows whose cached partner was i or j go on a list; j's members
//                 are relabelled in the same pass;
//              3. a wave per listed row rescans it.
//            Three barriers a step (none that costs anything in the single-wave form).
// Every loop's trip count is fixed by n_r when the block starts: at most n_r - 1 steps of a bounded number of strided passes.
// No block waits on another, there are no flags and no grid sync, and every index the kernel derives from data (a cached
// partner, a label, a list entry) is one it wrote itself from a loop counter below n_r: whatever S holds, NaN and infinities
// included, decides only WHICH in-range rows are touched.  The one LDS atomic is an integer counter (the list's length).
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_diar.h"
#include "diar_plan.h"
#include "host_support.h"

// The update is two products, a sum and a division, each rounded on its own: the merge list is compared bit by bit.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using diar_plan::mat_elems;

constexpr int kWave = XVEC_DIAR_RESCAN_WIDTH;
constexpr int kSmall = XVEC_DIAR_THREADS_SMALL;
constexpr int kLarge = XVEC_DIAR_THREADS_LARGE;
constexpr int kMaxSeg = XVEC_DIAR_MAX_SEGMENTS;
constexpr int kInitThreads = 256;
static_assert(kWave == 64 && kSmall == 64 && kLarge % 64 == 0 && kMaxSeg % kLarge == 0, "a wave per row, whole waves per block");

struct AhcArgs {
    const double* S;
    int64_t ld, N;
    int n_rec;
    const int64_t* rec_start;      // workspace copies
    const int* want;               // null: no recording asks for a count
    int64_t* mat_off;
    double* best_v;
    int* best_i;
    double* mats;
    double threshold;
    int max_clusters;
    int* labels;
    int* n_clusters;
    int* merge_i;                  // the three: all null or none
    int* merge_j;
    double* merge_score;
};

// A candidate: the score and the index it belongs to; i < 0 = none yet.  (v, i) comes before (b.v, b.i): larger score first,
// equal scores (-0.0 == +0.0) by lower index.  The caller keeps NaN out.
struct Best {
    double v;
    int i;
};

__device__ __forceinline__ bool before(double v, int i, const Best& b) { return b.i < 0 || v > b.v || (v == b.v && i < b.i); }

// The first of the wave's 64 candidates, in every lane (a total order on distinct indices: any order of combining gives it).
__device__ __forceinline__ Best wave_first(Best b) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(b.v, off);
        const int oi = __shfl_xor(b.i, off);
        if (oi >= 0 && before(ov, oi, b)) {
            b.v = ov;
            b.i = oi;
        }
    }
    return b;
}

// ---------------------------------------------------------------- layout

__global__ __launch_bounds__(256) void ahc_layout_kernel(const int64_t* __restrict__ rs, int n_rec, int64_t* __restrict__ mat_off) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = ((int64_t)n_rec + 255) / 256;
    const int64_t lo = t * per < n_rec ? t * per : n_rec, hi = lo + per < n_rec ? lo + per : n_rec;
    int64_t sum = 0;
    for (int64_t q = lo; q < hi; ++q) sum += mat_elems(rs[q + 1] - rs[q]);
    part[t] = sum;
    __syncthreads();
    int64_t at = 0;
    for (int u = 0; u < t; ++u) at += part[u];
    for (int64_t q = lo; q < hi; ++q) {
        mat_off[q] = at;
        at += mat_elems(rs[q + 1] - rs[q]);
    }
}

// ---------------------------------------------------------------- working copy and first bests

// The best partner of row k of a recording's working matrix among the cells c != k that `live` admits.  The cells are loaded
// BATCH at a time BEFORE they are judged (a dead column's cell is in range and merely ignored): a load behind its own test
// would wait for the one before it, and a row of 2048 cells would cost 32 memory latencies instead of 4.
template <int BATCH, typename Live>
__device__ __forceinline__ Best row_first(const double* __restrict__ row, int n, int k, int lane, Live live) {
    Best b{0.0, -1};
    for (int c0 = lane; c0 < n; c0 += BATCH * kWave) {
        double v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int c = c0 + u * kWave;
            v[u] = c < n ? row[c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int c = c0 + u * kWave;
            if (c >= n || c == k || !live(c)) continue;
            if (v[u] == v[u] && before(v[u], c, b)) {
                b.v = v[u];
                b.i = c;
            }
        }
    }
    return wave_first(b);
}

__global__ __launch_bounds__(kInitThreads) void ahc_init_kernel(const AhcArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * (kInitThreads / 64) + wave;
    if (row >= g.N) return;
    // the recording that owns the row: rec_start[lo] <= row < rec_start[hi] (rec_start increases strictly; 31 halvings at most)
    int lo = 0, hi = g.n_rec;
    for (int t = 0; t < 32 && hi - lo > 1; ++t) {
        const int mid = lo + (hi - lo) / 2;
        if (g.rec_start[mid] <= row) lo = mid; else hi = mid;
    }
    const int64_t start = g.rec_start[lo];
    const int n = (int)(g.rec_start[lo + 1] - start), a = (int)(row - start);
    if (n < 1 || n > kMaxSeg || a < 0 || a >= n) return;
    double* w = g.mats + g.mat_off[lo] + (int64_t)a * n;
    const double* sa = g.S + (start + a) * g.ld + start;      // row a of the block: cells right of the diagonal
    const double* sc = g.S + start * g.ld + start + a;        // column a of the block: cells above it
    for (int b = lane; b < n; b += kWave) {
        double v = std::numeric_limits<double>::quiet_NaN();
        if (b > a) v = sa[b];
        else if (b < a) v = sc[(int64_t)b * g.ld];
        w[b] = v;
    }
    // (each lane reads back the cells it wrote itself)
    const Best first = row_first<8>(w, n, a, lane, [](int) { return true; });
    if (lane == 0) {
        g.best_v[row] = first.v;
        g.best_i[row] = first.i;
    }
}

// ---------------------------------------------------------------- the merges

template <int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void ahc_cluster_kernel(const AhcArgs g, int rec0) {
    constexpr int WAVES = THREADS / 64;
    constexpr int kPass = CAP > THREADS ? 4 : 1;      // cells of row i a thread loads at a time in the update pass
    constexpr int kBatch = CAP > 64 ? 8 : 1;          // cells of a rescanned row a lane loads at a time
    __shared__ double bv[CAP];         // per live row: the score of its best partner ...
    __shared__ int bi[CAP];            // ... and the partner (-1: none selectable)
    __shared__ int sz[CAP];            // cluster size, 0 = merged away
    __shared__ int lab[CAP];           // per segment: the cluster it is in
    __shared__ int list[CAP];          // rows to rescan in this step
    __shared__ double red_v[2][WAVES];
    __shared__ int red_i[2][WAVES];
    __shared__ int nlist;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = rec0 + (int)blockIdx.x;
    const int64_t start = g.rec_start[r];
    const int n = (int)(g.rec_start[r + 1] - start);
    if (n < 1 || n > CAP || (n <= kSmall ? kSmall : kLarge) != THREADS) return;      // another launch's recording
    double* W = g.mats + g.mat_off[r];
    const int64_t ldw = n;                            // the working matrix is dense
    const int want = g.want ? g.want[r] : 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int k = tid; k < n; k += THREADS) {
        bv[k] = g.best_v[start + k];
        bi[k] = g.best_i[start + k];
        sz[k] = 1;
        lab[k] = k;
    }
    int steps = 0;
    for (; steps < n - 1; ++steps) {
        // 1. the pair to merge: the first of the live rows' cached bests
        Best b{0.0, -1};
        for (int k = tid; k < n; k += THREADS)
            if (sz[k] > 0 && bi[k] >= 0 && before(bv[k], k, b)) {
                b.v = bv[k];
                b.i = k;
            }
        b = wave_first(b);
        if (lane == 0) {
            red_v[0][wave] = b.v;
            red_i[0][wave] = b.i;
        }
        if (tid == 0) nlist = 0;
        __syncthreads();
        Best top{0.0, -1};
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
            if (red_i[0][w] >= 0 && before(red_v[0][w], red_i[0][w], top)) {
                top.v = red_v[0][w];
                top.i = red_i[0][w];
            }
        if (top.i < 0) break;                                   // one cluster left, or nothing but NaN pairs
        const int c = n - steps;
        const bool merge = want > 0 ? c > want : (top.v >= g.threshold || (g.max_clusters > 0 && c > g.max_clusters));
        if (!merge) break;
        const int i = top.i, j = bi[i];                         // i < j (see the head of the file)
        const double ni = (double)sz[i], nj = (double)sz[j], nn = (double)(sz[i] + sz[j]);
        const int merged = sz[i] + sz[j];

        // 2. row i and column i become the merged cluster's; every other live row looks at its new cell
        double* Wi = W + i * ldw;
        const double* Wj = W + j * ldw;
        Best mine{0.0, -1};
        for (int k0 = tid; k0 < n; k0 += kPass * THREADS) {
            double si[kPass], sj[kPass];                        // loaded before they are judged, as in row_first
#pragma unroll
            for (int u = 0; u < kPass; ++u) {
                const int k = k0 + u * THREADS;
                si[u] = k < n ? Wi[k] : 0.0;
                sj[u] = k < n ? Wj[k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kPass; ++u) {
                const int k = k0 + u * THREADS;
                if (k >= n) continue;
                if (lab[k] == j) lab[k] = i;
                if (k == i || k == j || sz[k] <= 0) continue;
                const double v = (ni * si[u] + nj * sj[u]) / nn;
                Wi[k] = v;
                W[k * ldw + i] = v;
                const bool ok = v == v;
                if (ok && before(v, k, mine)) {
                    mine.v = v;
                    mine.i = k;
                }
                const int old = bi[k];
                if (old == i || old == j) {
                    list[atomicAdd(&nlist, 1)] = k;             // at most n - 2 entries: one per k
                } else if (ok && before(v, i, Best{bv[k], old})) {
                    bv[k] = v;
                    bi[k] = i;
                }
            }
        }
        mine = wave_first(mine);
        if (lane == 0) {
            red_v[1][wave] = mine.v;
            red_i[1][wave] = mine.i;
        }
        __syncthreads();
        if (tid == 0) {
            Best row{0.0, -1};
#pragma unroll
            for (int w = 0; w < WAVES; ++w)
                if (red_i[1][w] >= 0 && before(red_v[1][w], red_i[1][w], row)) {
                    row.v = red_v[1][w];
                    row.i = red_i[1][w];
                }
            bv[i] = row.v;
            bi[i] = row.i;
            sz[i] = merged;
            sz[j] = 0;
            if (g.merge_i) {
                g.merge_i[start + steps] = i;
                g.merge_j[start + steps] = j;
                g.merge_score[start + steps] = top.v;
            }
        }

        // 3. the rows that lost their partner: a wave each (i is live and j is not, whatever thread 0 has written of them yet)
        const int todo = nlist;
        for (int q = wave; q < todo; q += WAVES) {
            const int k = list[q];
            const Best first = row_first<kBatch>(W + k * ldw, n, k, lane, [&](int c2) { return c2 == i || (c2 != j && sz[c2] > 0); });
            if (lane == 0) {
                bv[k] = first.v;
                bi[k] = first.i;
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // clusters numbered in the order of their lowest segment, which is their name: rank = live rows below (wave 0, by ballot)
    if (wave == 0) {
        int seen = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool alive = k < n && sz[k] > 0;
            const unsigned long long m = __ballot(alive);
            if (alive) bi[k] = seen + __popcll(m & ((1ull << lane) - 1ull));
            seen += __popcll(m);
        }
        if (lane == 0) g.n_clusters[r] = seen;
    }
    __syncthreads();
    for (int k = tid; k < n; k += THREADS) {
        g.labels[start + k] = bi[lab[k]];
        if (g.merge_i && k >= steps) {                          // the merges not performed, and the recording's last slot
            g.merge_i[start + k] = -1;
            g.merge_j[start + k] = -1;
            g.merge_score[start + k] = nan;
        }
    }
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_derr;

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_diar_last_error(void) { return g_derr.c_str(); }

size_t xvec_ahc_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec) {
    Refusal why;
    if (diar_plan::check_rec_start(rec_start_host, n_rec, why)) return 0;
    return diar_plan::make_layout(rec_start_host, n_rec).total;
}

int xvec_ahc_cluster(const double* S, int64_t ld, const int64_t* rec_start_host, int32_t n_rec, double threshold,
                     int32_t max_clusters, const int32_t* want_host, int32_t* labels, int32_t* n_clusters, int32_t* merge_i,
                     int32_t* merge_j, double* merge_score, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    if (diar_plan::check_rec_start(rec_start_host, n_rec, why)) return g_derr.refused(XVEC_ERR_ARG, why);
    const int64_t N = rec_start_host[n_rec];
    if (threshold != threshold) return g_derr.fail(XVEC_ERR_ARG, "threshold is NaN (+inf never merges by score, -inf always)");
    if (max_clusters < 0) return g_derr.fail(XVEC_ERR_ARG, "max_clusters = %d must not be negative (0 = no limit)", max_clusters);
    if (diar_plan::check_want(want_host, n_rec, why)) return g_derr.refused(XVEC_ERR_ARG, why);
    if (ld < N) return g_derr.fail(XVEC_ERR_ARG, "ld = %lld is smaller than the %lld segments", (long long)ld, (long long)N);
    if (!S || !labels || !n_clusters) return g_derr.fail(XVEC_ERR_ARG, "null pointer: S / labels / n_clusters");
    if (!(merge_i && merge_j && merge_score) && (merge_i || merge_j || merge_score))
        return g_derr.fail(XVEC_ERR_ARG, "merge_i, merge_j and merge_score: all three or none");
    const diar_plan::Layout l = diar_plan::make_layout(rec_start_host, n_rec);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_derr))) return rc;

    AhcArgs g{};
    g.S = S;
    g.ld = ld;
    g.N = N;
    g.n_rec = n_rec;
    g.rec_start = part<const int64_t>(workspace, l.rec_start);
    g.want = want_host ? part<const int>(workspace, l.want) : nullptr;
    g.mat_off = part<int64_t>(workspace, l.mat_off);
    g.best_v = part<double>(workspace, l.best_v);
    g.best_i = part<int>(workspace, l.best_i);
    g.mats = part<double>(workspace, l.mats);
    g.threshold = threshold;
    g.max_clusters = max_clusters;
    g.labels = labels;
    g.n_clusters = n_clusters;
    g.merge_i = merge_i;
    g.merge_j = merge_j;
    g.merge_score = merge_score;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const char* copied = "rec_start / want";
    if ((rc = upload(part<int64_t>(workspace, l.rec_start), rec_start_host, (size_t)n_rec + 1, copied, s, g_derr))) return rc;
    if (want_host && (rc = upload(part<int32_t>(workspace, l.want), want_host, (size_t)n_rec, copied, s, g_derr))) return rc;
    ahc_layout_kernel<<<1, 256, 0, s>>>(g.rec_start, n_rec, g.mat_off);
    if ((rc = g_derr.launch_ok("ahc_layout_kernel"))) return rc;
    constexpr int rows = kInitThreads / 64;
    ahc_init_kernel<<<(unsigned)((N + rows - 1) / rows), kInitThreads, 0, s>>>(g);
    if ((rc = g_derr.launch_ok("ahc_init_kernel"))) return rc;
    diar_plan::Group groups[2];
    const int n_groups = diar_plan::plan_groups(rec_start_host, n_rec, groups);
    for (int q = 0; q < n_groups; ++q) {
        const diar_plan::Group& grp = groups[q];
        if (grp.threads == kSmall)
            ahc_cluster_kernel<kSmall, kSmall><<<(unsigned)grp.count, kSmall, 0, s>>>(g, grp.first);
        else
            ahc_cluster_kernel<kLarge, kMaxSeg><<<(unsigned)grp.count, kLarge, 0, s>>>(g, grp.first);
        if ((rc = g_derr.launch_ok("ahc_cluster_kernel"))) return rc;
    }
    return XVEC_OK;
}

}  // extern "C"
