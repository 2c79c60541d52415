// DER scoring: the diarization error rate of hypothesis turns against reference turns with the optimal speaker mapping.
// C ABI, the definition and its rules: include/xvec_der.h; the host-only half (checks, workspace layout, launch plan):
// der_plan.h.
//   raster   a wave per turn of either side: its speaker bit ORed into the per-tick 64-bit masks and, for a reference turn,
//            its two collar zones into the no-score bitmap (integer OR atomics commute: the order of the turns cannot show).
//            One block more lays out blk_start, the first block of every recording in the pass.
//   pass     a block per XVEC_DER_CHUNK_TICKS consecutive ticks of one recording; each wave walks XVEC_DER_WAVE_ROWS rows of 64
//            consecutive ticks, a lane per tick (512 contiguous bytes a load).  Speech comes in long runs of one (R_t, H_t)
//            pair: with an LDS atomic per tick all 64 lanes of a wave would hit one address for thousands of ticks.  So the
//            lanes compare their pair with their neighbour's, a vote marks where the runs of the row begin, and only the first
//            lane of a run touches the block's 64 x 64 LDS histogram, with the run's length (k * l updates for a pair of k and l
//            speakers).  The block adds the cells it touched to the recording's int64 matrix with integer atomics.
//   assign   a wave per recording, a lane per hypothesis speaker: shortest augmenting paths (Hungarian / Jonker-Volgenant) on
//            int64 potentials over the rows that have a positive entry, the matrix in LDS as 32-bit values.  The column with
//            the smallest reduced cost is found by a butterfly over (cost << 6 | lane): ties go to the lowest lane, so the map
//            is a function of C alone.  Then conf, der and the copies out.
//   pool     one block: the batch's summed errors over its summed totals.
// Every loop of the solver runs a counter to 64 at most, whatever the data: a step marks one more of the 64 columns, a path
// has 64 columns at most.  No block waits on another; every index is a loop counter, a checked turn field or a lane number
// taken from the low six bits of a value.  Integer atomics only.
#include <hip/hip_runtime.h>

#include "../../include/xvec_der.h"
#include "../../include/xvec_hip.h"
#include "der_plan.h"
#include "host_support.h"

namespace xvec {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kThreads = XVEC_DER_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = XVEC_DER_WAVE_ROWS;
constexpr int kChunk = XVEC_DER_CHUNK_TICKS;
constexpr int kSpk = XVEC_DER_MAX_SPEAKERS;
constexpr int kCells = kSpk * kSpk;
static_assert(kSpk == 64 && kChunk == kThreads * kRows && kRows <= 32 && kCells % kThreads == 0, "a lane per speaker, the waves' rows tile a chunk");

struct RasterArgs {
    const int* ref;
    i64 m_ref;
    const int* hyp;
    i64 m_hyp;
    const i64* rec_start;      // the workspace copy
    int n_rec;
    int collar;
    u64* ref_mask;
    u64* hyp_mask;
    unsigned* noscore;
    u64* ignored;
    int* blk_start;
};

struct PassArgs {
    const i64* rec_start;
    const int* blk_start;
    int n_rec;
    int skip_overlap;
    const u64* ref_mask;
    const u64* hyp_mask;
    const unsigned* noscore;
    u64* acc;                  // [n_rec, 4]: scored, total, miss, fa
    u64* cooc;                 // [n_rec, 64, 64]
};

struct AssignArgs {
    const i64* cooc_in;        // [n_rec, 64, 64]
    i64* cooc_out;             // may be null
    const i64* acc;            // null for xvec_der_assign
    const i64* ign;            // the workspace's [2]; null for xvec_der_assign
    i64* counts;               // [n_rec, 4] without a map, [n_rec, 5] with one; null for xvec_der_assign
    int* map;                  // null: no solver (xvec_der_cooccurrence)
    i64* correct;              // may be null
    double* der;               // may be null
    i64* ignored_out;          // may be null
};

__device__ __forceinline__ i64 chunks_of(i64 ticks) { return (ticks + kChunk - 1) / kChunk; }

// ---------------------------------------------------------------- raster

__global__ __launch_bounds__(kThreads) void der_raster_kernel(RasterArgs a) {
    __shared__ int sPart[kThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        // blk_start: thread t sums the chunks of its stretch of recordings, thread 0 scans the 256 sums
        const int per = (a.n_rec + kThreads - 1) / kThreads;
        const i64 lo = (i64)tid * per < a.n_rec ? (i64)tid * per : a.n_rec, hi = lo + per < a.n_rec ? lo + per : a.n_rec;
        int sum = 0;
        for (i64 r = lo; r < hi; ++r) sum += (int)chunks_of(a.rec_start[r + 1] - a.rec_start[r]);
        sPart[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int t = 0; t < kThreads; ++t) {
                const int s = sPart[t];
                sPart[t] = run;
                run += s;
            }
            a.blk_start[a.n_rec] = run;
        }
        __syncthreads();
        int at = sPart[tid];
        for (i64 r = lo; r < hi; ++r) {
            a.blk_start[r] = at;
            at += (int)chunks_of(a.rec_start[r + 1] - a.rec_start[r]);
        }
        return;
    }
    const i64 w = (i64)blockIdx.x * kWaves + wave;
    if (w >= a.m_ref + a.m_hyp) return;
    const bool is_ref = w < a.m_ref;
    const int* row = is_ref ? a.ref + 4 * w : a.hyp + 4 * (w - a.m_ref);
    const int rec = row[0], start = row[1], end = row[2], spk = row[3];
    if (rec < 0 || rec >= a.n_rec || spk < 0 || spk >= kSpk || end <= start) {
        if (lane == 0) atomicAdd(&a.ignored[is_ref ? 0 : 1], 1ull);
        return;
    }
    const i64 base = a.rec_start[rec], n = a.rec_start[rec + 1] - base;
    const i64 s = start > 0 ? start : 0, e = end < n ? end : n;
    u64* mask = (is_ref ? a.ref_mask : a.hyp_mask) + base;
    const u64 bit = 1ull << spk;
    for (i64 t = s + lane; t < e; t += 64) atomicOr(&mask[t], bit);
    if (!is_ref || a.collar == 0) return;
    for (int k = 0; k < 2; ++k) {
        const i64 b = k ? end : start;
        const i64 zlo = b - a.collar > 0 ? b - a.collar : 0, zhi = b + a.collar < n ? b + a.collar : n;
        if (zlo >= zhi) continue;
        const i64 glo = base + zlo, glast = base + zhi - 1;            // bits glo .. glast of the bitmap
        const i64 first = glo >> 5, last = glast >> 5;
        for (i64 wd = first + lane; wd <= last; wd += 64) {
            unsigned m = ~0u;
            if (wd == first) m &= ~0u << (glo & 31);
            if (wd == last) m &= ~0u >> (31 - (glast & 31));
            atomicOr(&a.noscore[wd], m);
        }
    }
}

// ---------------------------------------------------------------- pass

// `run` ticks of the pair (R, H) into the block's histogram: nothing for a pair with an empty side.
__device__ __forceinline__ void flush_run(unsigned* hist, u64 R, u64 H, unsigned run) {
    if (R == 0 || H == 0) return;
    for (int x = 0; x < kSpk && R; ++x) {
        const int i = __ffsll((i64)R) - 1;
        R &= R - 1;
        u64 h = H;
        for (int y = 0; y < kSpk && h; ++y) {
            const int j = __ffsll((i64)h) - 1;
            h &= h - 1;
            atomicAdd(&hist[i * kSpk + j], run);
        }
    }
}

__global__ __launch_bounds__(kThreads) void der_pass_kernel(PassArgs a) {
    __shared__ unsigned sHist[kCells];
    __shared__ unsigned sCnt[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < kCells; i += kThreads) sHist[i] = 0;
    if (tid < 4) sCnt[tid] = 0;
    // the block's recording: blk_start[r] <= block < blk_start[r + 1], by bisection
    const int block = (int)blockIdx.x;
    int lo = 0, hi = a.n_rec;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.blk_start[mid] <= block) lo = mid; else hi = mid;
    }
    const int r = lo;
    const i64 base = a.rec_start[r], n = a.rec_start[r + 1] - base;
    const int lane = tid & 63, wave = tid >> 6;
    const i64 w0 = (i64)(block - a.blk_start[r]) * kChunk + (i64)wave * (kRows * 64);      // the wave's first tick
    __syncthreads();
    unsigned scored = 0, total = 0, miss = 0, fa = 0;
#pragma unroll 4
    for (int q = 0; q < kRows; ++q) {
        if (w0 + q * 64 >= n) break;                 // the same in every lane
        const i64 t = w0 + q * 64 + lane;
        u64 R = 0, H = 0;                            // an unscored tick and a tick behind the recording: the empty pair
        if (t < n) {
            const i64 g = base + t;
            R = a.ref_mask[g];
            H = a.hyp_mask[g];
            const unsigned ns = (a.noscore[g >> 5] >> (g & 31)) & 1u;
            const int nr = __popcll(R), nh = __popcll(H);
            if (ns || (a.skip_overlap && nr > 1)) {
                R = 0;
                H = 0;
            } else {
                scored += 1;
                total += nr;
                miss += nr > nh ? nr - nh : 0;
                fa += nh > nr ? nh - nr : 0;
            }
        }
        // the runs of one pair along the row: the first lane of a run adds the run's length, the others add nothing
        const u64 pR = __shfl_up(R, 1), pH = __shfl_up(H, 1);
        const bool head = lane == 0 || R != pR || H != pH;
        const u64 heads = __ballot(head);
        if (head && R && H) {
            const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);
            flush_run(sHist, R, H, rest ? (unsigned)__ffsll((i64)rest) : (unsigned)(64 - lane));
        }
    }
    if (scored) atomicAdd(&sCnt[0], scored);
    if (total) atomicAdd(&sCnt[1], total);
    if (miss) atomicAdd(&sCnt[2], miss);
    if (fa) atomicAdd(&sCnt[3], fa);
    __syncthreads();
    u64* C = a.cooc + (size_t)r * kCells;
    for (int i = tid; i < kCells; i += kThreads) {
        const unsigned v = sHist[i];
        if (v) atomicAdd(&C[i], (u64)v);
    }
    if (tid < 4 && sCnt[tid]) atomicAdd(&a.acc[(size_t)r * 4 + tid], (u64)sCnt[tid]);
}

// ---------------------------------------------------------------- assign

__device__ __forceinline__ int lane_value(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

__device__ __forceinline__ i64 lane_value(i64 v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u64)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((u64)v >> 32), src);
    return (i64)(((u64)hi << 32) | lo);
}

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ i64 wave_sum(i64 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(64) void der_assign_kernel(AssignArgs a) {
    __shared__ unsigned sC[kCells];
    __shared__ int sInv[kSpk];
    const int r = (int)blockIdx.x, j = (int)threadIdx.x;
    const i64* C = a.cooc_in + (size_t)r * kCells;
    i64* Cout = a.cooc_out ? a.cooc_out + (size_t)r * kCells : nullptr;
    u64 rows = 0;                                    // bit i: row i has a positive entry (the same in every lane)
    for (int i = 0; i < kSpk; ++i) {
        const i64 c = C[i * kSpk + j];
        if (Cout) Cout[i * kSpk + j] = c;
        sC[i * kSpk + j] = (unsigned)c;
        if (__ballot((unsigned)c != 0u)) rows |= 1ull << i;
    }
    sInv[j] = -1;
    __syncthreads();
    i64 correct = 0;
    if (a.map) {
        // minimise sum (2^32 - 1 - C) over the rows with an entry: every such row gets a column, so the constant does not move
        // the optimum, and costs, reduced costs and potentials stay in 0 .. 2^39.  Lane j is COLUMN j (v, p = its row or -1, and per root minv, way,
        // used) and ROW j (u, in_tree).
        i64 u = 0, v = 0;
        int p = -1;
        for (int i = 0; i < kSpk; ++i) {
            if (!((rows >> i) & 1ull)) continue;
            i64 minv = 0x7fffffffffffffffll;
            int way = -1;                            // the column in front of this one on its path; -1: the root row
            bool used = false, in_tree = j == i;
            int i0 = i, j0 = -1, leaf = -1;
            for (int step = 0; step < kSpk; ++step) {        // a step marks one more column: 64 at most
                const i64 ui0 = lane_value(u, i0);
                if (!used) {
                    const i64 cur = (i64)(0xffffffffu - sC[i0 * kSpk + j]) - ui0 - v;
                    if (cur < minv) {
                        minv = cur;
                        way = j0;
                    }
                }
                const u64 key = wave_min(used ? ~0ull : (((u64)minv << 6) | (u64)j));
                const int j1 = __builtin_amdgcn_readfirstlane((int)(key & 63ull));
                const i64 delta = lane_value(minv, j1);
                if (in_tree) u += delta;
                if (used) v -= delta; else minv -= delta;
                const int pj1 = lane_value(p, j1);
                if (j == j1) used = true;
                j0 = j1;
                if (pj1 < 0) {
                    leaf = j1;
                    break;
                }
                i0 = pj1 & 63;
                if (j == i0) in_tree = true;
            }
            for (int k = 0, jc = leaf; k < kSpk && jc >= 0; ++k) {      // back along the path: 64 columns at most
                const int jp = lane_value(way, jc);
                const int up = lane_value(p, jp & 63);
                if (j == jc) p = jp < 0 ? i : up;
                jc = jp < 0 ? -1 : (jp & 63);
            }
        }
        i64 mine = 0;
        if (p >= 0) {
            const unsigned c = sC[(p & 63) * kSpk + j];
            if (c) {                                 // a pair that never met is not reported
                sInv[p & 63] = j;
                mine = c;
            }
        }
        __syncthreads();
        a.map[(size_t)r * kSpk + j] = sInv[j];
        correct = wave_sum(mine);
        if (a.correct && j == 0) a.correct[r] = correct;
    }
    if (a.counts) {
        const i64* acc = a.acc + (size_t)r * 4;
        if (!a.map) {
            if (j < 4) a.counts[(size_t)r * 4 + j] = acc[j];
        } else if (j == 0) {
            const i64 scored = acc[0], total = acc[1], miss = acc[2], fa = acc[3];
            const i64 conf = total - miss - correct;              // sum min(Nref, Nhyp) = total - miss
            i64* out = a.counts + (size_t)r * 5;
            out[0] = scored;
            out[1] = total;
            out[2] = miss;
            out[3] = fa;
            out[4] = conf;
            if (a.der) a.der[r] = total ? (double)(miss + fa + conf) / (double)total : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    if (a.ignored_out && r == 0 && j < 2) a.ignored_out[j] = a.ign[j];
}

// ---------------------------------------------------------------- pool

__global__ __launch_bounds__(kThreads) void der_pool_kernel(const i64* counts, int n_rec, double* der) {
    __shared__ u64 sSum[2];
    const int tid = threadIdx.x;
    if (tid < 2) sSum[tid] = 0;
    __syncthreads();
    u64 err = 0, total = 0;
    for (int r = tid; r < n_rec; r += kThreads) {
        const i64* c = counts + (size_t)r * 5;
        total += (u64)c[1];
        err += (u64)(c[2] + c[3] + c[4]);
    }
    if (err) atomicAdd(&sSum[0], err);
    if (total) atomicAdd(&sSum[1], total);
    __syncthreads();
    if (tid == 0) der[n_rec] = sSum[1] ? (double)(i64)sSum[0] / (double)(i64)sSum[1] : __longlong_as_double(0x7ff8000000000000ll);
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_derr;

// What xvec_der_cooccurrence and xvec_der_score share: the checks, the copy of rec_start, the zeroing, raster and pass.
int front(const int32_t* ref_turns, int64_t m_ref, const int32_t* hyp_turns, int64_t m_hyp, const int64_t* rec_start_host,
          int32_t n_rec, int32_t collar, int32_t skip_overlap, bool outputs_given, const char* outputs, void* workspace,
          size_t workspace_bytes, hipStream_t s, der_plan::Layout& l) {
    Refusal why;
    if (der_plan::check_rec_start(rec_start_host, n_rec, why) || der_plan::check_turn_counts(m_ref, m_hyp, why) ||
        der_plan::check_collar(collar, why) || der_plan::check_turns(ref_turns, m_ref, "ref", why) ||
        der_plan::check_turns(hyp_turns, m_hyp, "hyp", why))
        return g_derr.refused(XVEC_ERR_ARG, why);
    if (!outputs_given) return g_derr.fail(XVEC_ERR_ARG, "null pointer: %s", outputs);
    l = der_plan::make_layout(rec_start_host, n_rec);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_derr))) return rc;
    if ((rc = upload(part<int64_t>(workspace, l.rec_start), rec_start_host, (size_t)n_rec + 1, "rec_start", s, g_derr)))
        return rc;
    const hipError_t e = hipMemsetAsync(part<char>(workspace, l.zero_from), 0, l.total - l.zero_from, s);
    if (e != hipSuccess) return g_derr.fail(XVEC_ERR_HIP, "zeroing the workspace failed: %s", hipGetErrorString(e));

    RasterArgs ra{};
    ra.ref = ref_turns;
    ra.m_ref = m_ref;
    ra.hyp = hyp_turns;
    ra.m_hyp = m_hyp;
    ra.rec_start = part<const i64>(workspace, l.rec_start);
    ra.n_rec = n_rec;
    ra.collar = collar;
    ra.ref_mask = part<u64>(workspace, l.ref_mask);
    ra.hyp_mask = part<u64>(workspace, l.hyp_mask);
    ra.noscore = part<unsigned>(workspace, l.noscore);
    ra.ignored = part<u64>(workspace, l.ignored);
    ra.blk_start = part<int>(workspace, l.blk_start);
    const der_plan::Launch rl = der_plan::raster_launch(m_ref, m_hyp);
    der_raster_kernel<<<(unsigned)rl.blocks, rl.threads, 0, s>>>(ra);
    if ((rc = g_derr.launch_ok("der_raster_kernel"))) return rc;

    PassArgs pa{};
    pa.rec_start = ra.rec_start;
    pa.blk_start = ra.blk_start;
    pa.n_rec = n_rec;
    pa.skip_overlap = skip_overlap ? 1 : 0;
    pa.ref_mask = ra.ref_mask;
    pa.hyp_mask = ra.hyp_mask;
    pa.noscore = ra.noscore;
    pa.acc = part<u64>(workspace, l.acc);
    pa.cooc = part<u64>(workspace, l.cooc);
    const der_plan::Launch pl = der_plan::pass_launch(rec_start_host, n_rec);
    der_pass_kernel<<<(unsigned)pl.blocks, pl.threads, 0, s>>>(pa);
    return g_derr.launch_ok("der_pass_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_der_last_error(void) { return g_derr.c_str(); }

size_t xvec_der_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec, int64_t m_ref, int64_t m_hyp) {
    Refusal why;
    if (der_plan::check_rec_start(rec_start_host, n_rec, why) || der_plan::check_turn_counts(m_ref, m_hyp, why)) return 0;
    return der_plan::make_layout(rec_start_host, n_rec).total;
}

int xvec_der_cooccurrence(const int32_t* ref_turns, int64_t m_ref, const int32_t* hyp_turns, int64_t m_hyp,
                          const int64_t* rec_start_host, int32_t n_rec, int32_t collar, int32_t skip_overlap, int64_t* counts,
                          int64_t* cooc, int64_t* ignored, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    der_plan::Layout l{};
    int rc;
    if ((rc = front(ref_turns, m_ref, hyp_turns, m_hyp, rec_start_host, n_rec, collar, skip_overlap, counts && cooc && ignored,
                    "counts / cooc / ignored", workspace, workspace_bytes, s, l)))
        return rc;
    AssignArgs g{};
    g.cooc_in = part<const i64>(workspace, l.cooc);
    g.cooc_out = reinterpret_cast<i64*>(cooc);
    g.acc = part<const i64>(workspace, l.acc);
    g.ign = part<const i64>(workspace, l.ignored);
    g.counts = reinterpret_cast<i64*>(counts);
    g.ignored_out = reinterpret_cast<i64*>(ignored);
    const der_plan::Launch al = der_plan::assign_launch(n_rec);
    der_assign_kernel<<<(unsigned)al.blocks, al.threads, 0, s>>>(g);
    return g_derr.launch_ok("der_assign_kernel");
}

int xvec_der_assign(const int64_t* cooc, int32_t n_rec, int32_t* map, int64_t* correct, xvec_stream stream) {
    if (n_rec < 1) return g_derr.fail(XVEC_ERR_ARG, "n_rec = %d: need at least one recording", n_rec);
    if (!cooc || !map || !correct) return g_derr.fail(XVEC_ERR_ARG, "null pointer: cooc / map / correct");
    AssignArgs g{};
    g.cooc_in = reinterpret_cast<const i64*>(cooc);
    g.map = map;
    g.correct = reinterpret_cast<i64*>(correct);
    const der_plan::Launch al = der_plan::assign_launch(n_rec);
    der_assign_kernel<<<(unsigned)al.blocks, al.threads, 0, static_cast<hipStream_t>(stream)>>>(g);
    return g_derr.launch_ok("der_assign_kernel");
}

int xvec_der_score(const int32_t* ref_turns, int64_t m_ref, const int32_t* hyp_turns, int64_t m_hyp,
                   const int64_t* rec_start_host, int32_t n_rec, int32_t collar, int32_t skip_overlap, int64_t* counts,
                   int32_t* map, double* der, int64_t* ignored, int64_t* cooc, void* workspace, size_t workspace_bytes,
                   xvec_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    der_plan::Layout l{};
    int rc;
    if ((rc = front(ref_turns, m_ref, hyp_turns, m_hyp, rec_start_host, n_rec, collar, skip_overlap, counts && map && der && ignored,
                    "counts / map / der / ignored", workspace, workspace_bytes, s, l)))
        return rc;
    AssignArgs g{};
    g.cooc_in = part<const i64>(workspace, l.cooc);
    g.cooc_out = reinterpret_cast<i64*>(cooc);
    g.acc = part<const i64>(workspace, l.acc);
    g.ign = part<const i64>(workspace, l.ignored);
    g.counts = reinterpret_cast<i64*>(counts);
    g.map = map;
    g.der = der;
    g.ignored_out = reinterpret_cast<i64*>(ignored);
    const der_plan::Launch al = der_plan::assign_launch(n_rec);
    der_assign_kernel<<<(unsigned)al.blocks, al.threads, 0, s>>>(g);
    if ((rc = g_derr.launch_ok("der_assign_kernel"))) return rc;
    const der_plan::Launch ql = der_plan::pool_launch();
    der_pool_kernel<<<(unsigned)ql.blocks, ql.threads, 0, s>>>(reinterpret_cast<const i64*>(counts), n_rec, der);
    return g_derr.launch_ok("der_pool_kernel");
}

}  // extern "C"
