// The radix sort of the trial family: (key, payload) pairs by key, stable, least significant digit first, 4 passes of 8 bits.
// Per pass: per-tile digit histogram, scan of the histograms, scatter that ranks inside the tile with wave ballots and reorders
// through LDS.  ONE sort, templated over the payload that travels with each key: eval.hip (and through it calibration and the
// report) carries the target bit, one byte; boot.hip carries 32 bits (the trial's index, or its packed group ids), and
// xvec_eval_sorted_order (include/xvec_eval.h) is that instantiation.  A translation unit compiles the instantiations it uses.
// After <hip/hip_runtime.h>, host_support.h and trial_device.h.
#pragma once
#include <algorithm>
#include <cstdint>

#include "host_support.h"
#include "trial_device.h"

namespace xvec {
namespace trial_sort {

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;      // elements a block owns in every stage
constexpr int kWaves = kThreads / 64;
constexpr int kRadix = 256;                   // 8-bit digits

inline int64_t chunks(int64_t len) { return (len + kTile - 1) / kTile; }

// The buffers of one sort of n pairs: keys / pay ping and pong (the sorted pairs end in [0]), hist [chunks(n) * kRadix],
// hist_sums [chunks(chunks(n) * kRadix)].
template <typename P>
struct SortBufs {
    uint32_t* keys[2];
    P* pay[2];
    uint32_t *hist, *hist_sums;
};

// sorted_order's part of xvec_eval_sorted_order: defined in boot.hip, where the 32-bit instantiation is compiled.  The
// workspace holds sorted_order_bytes(n); keys_out / order_out [n] as include/xvec_eval.h states them.
size_t sorted_order_bytes(int64_t n);
int sorted_order(const trial_device::TrialArgs& trials, bool all_pairs, uint32_t* keys_out, uint32_t* order_out, void* workspace, hipStream_t s,
                 ErrorChannel& err);

namespace {

using trial_device::block_excl_scan;
using trial_device::block_scan_array;

// hist[digit * num_tiles + tile] = elements of the tile with that digit (digit-major: one scan of the whole table gives every
// (digit, tile) its first output position)
__global__ __launch_bounds__(kThreads) void eval_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                             uint32_t* __restrict__ hist, int num_tiles) {
    __shared__ uint32_t h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRadix - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * num_tiles + blockIdx.x] = h[threadIdx.x];
}

// In-place exclusive scan of a uint32 array of any length, three launches: chunk sums, scan of the chunk sums (one block),
// scan of every chunk with its offset.  A chunk is kTile elements.
__global__ __launch_bounds__(kThreads) void eval_scan_sums_kernel(const uint32_t* __restrict__ v, int64_t len,
                                                                  uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t s = 0;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < len) s += v[i];
    }
    uint32_t total;
    block_excl_scan(s, wtot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void eval_scan_top_kernel(uint32_t* __restrict__ sums, int64_t n_sums,
                                                                 unsigned long long* __restrict__ total_out) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t total = block_scan_array(sums, sums, n_sums, wtot);
    if (total_out && threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kThreads) void eval_scan_apply_kernel(uint32_t* __restrict__ v, int64_t len,
                                                                   const uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    uint32_t x[kItems], s = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        x[k] = base + k < len ? v[base + k] : 0u;
        s += x[k];
    }
    uint32_t run = block_excl_scan(s, wtot, nullptr) + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (base + k < len) v[base + k] = run;
        run += x[k];
    }
}

// One pass: the tile's elements, in input order, go to offs[digit][tile] + (rank among the tile's elements of that digit).
// Wave w owns the elements [w * 1024, (w + 1) * 1024) of the tile, 64 at a time: the lanes with the same digit find each other
// with eight ballots, rank = that wave's count of the digit so far + lanes below.  The tile is then laid out in digit order in
// LDS and written from there, so that neighbouring threads write neighbouring addresses within each digit's run.
template <typename P>
__global__ __launch_bounds__(kThreads) void eval_scatter_kernel(const uint32_t* __restrict__ kin, const P* __restrict__ bin,
                                                                uint32_t* __restrict__ kout, P* __restrict__ bout, int64_t n,
                                                                int shift, const uint32_t* __restrict__ offs, int num_tiles) {
    __shared__ uint32_t wcnt[kWaves][kRadix];     // per wave: running count of each digit, then the wave's base inside the digit
    __shared__ uint32_t dstart[kRadix];           // first tile-local position of each digit
    __shared__ uint32_t goff[kRadix];             // first output position of each digit of this tile
    __shared__ uint32_t wtot[kWaves];
    __shared__ uint32_t skey[kTile];
    __shared__ P sbit[kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
    const int cnt = (int)std::min<int64_t>(kTile, n - base);
    const uint64_t below_mask = (1ull << lane) - 1ull;

    uint32_t key[kItems], rank[kItems];
    P bit[kItems];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int li = wave * (64 * kItems) + r * 64 + lane;
        const bool active = li < cnt;
        key[r] = active ? kin[base + li] : 0u;
        bit[r] = active ? bin[base + li] : (P)0;
        const uint32_t d = (key[r] >> shift) & (kRadix - 1);
        uint64_t peers = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool set = (d >> b) & 1u;
            const uint64_t bal = __ballot(set);
            peers &= set ? bal : ~bal;
        }
        const uint32_t below = (uint32_t)__popcll(peers & below_mask);
        const uint32_t prev = active ? wcnt[wave][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (active && below == 0) wcnt[wave][d] = prev + (uint32_t)__popcll(peers);     // the lowest lane of each digit
        __builtin_amdgcn_wave_barrier();
        rank[r] = prev + below;
    }
    __syncthreads();
    {   // thread = digit: the waves' counts -> each wave's base inside the digit; digit totals -> tile-local starts
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t c = wcnt[w][tid];
            wcnt[w][tid] = run;
            run += c;
        }
        dstart[tid] = block_excl_scan(run, wtot, nullptr);
        goff[tid] = offs[(size_t)tid * num_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int li = wave * (64 * kItems) + r * 64 + lane;
        if (li < cnt) {
            const uint32_t d = (key[r] >> shift) & (kRadix - 1);
            const uint32_t p = dstart[d] + wcnt[wave][d] + rank[r];
            if (p < (uint32_t)kTile) {      // always true: a bound, not a branch taken
                skey[p] = key[r];
                sbit[p] = bit[r];
            }
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int p = k * kThreads + tid;
        if (p < cnt) {
            const uint32_t kk = skey[p];
            const uint32_t d = (kk >> shift) & (kRadix - 1);
            const int64_t pos = (int64_t)goff[d] + (int64_t)(p - (int)dstart[d]);
            if (pos >= 0 && pos < n) {      // always true when offs is the scan of this pass's histogram
                kout[pos] = kk;
                bout[pos] = sbit[p];
            }
        }
    }
}

// v[0 .. len) <- its exclusive scan; *total_out (device, may be null) <- the sum
inline int scan_in_place(uint32_t* v, int64_t len, uint32_t* sums, unsigned long long* total_out, hipStream_t s,
                         ErrorChannel& err) {
    const int64_t nc = chunks(len);
    int rc;
    eval_scan_sums_kernel<<<(unsigned)nc, kThreads, 0, s>>>(v, len, sums);
    if ((rc = err.launch_ok("eval_scan_sums_kernel"))) return rc;
    eval_scan_top_kernel<<<1, kThreads, 0, s>>>(sums, nc, total_out);
    if ((rc = err.launch_ok("eval_scan_top_kernel"))) return rc;
    eval_scan_apply_kernel<<<(unsigned)nc, kThreads, 0, s>>>(v, len, sums);
    return err.launch_ok("eval_scan_apply_kernel");
}

// The four passes over the n pairs in keys[0] / pay[0]; the sorted pairs end there again.
template <typename P>
inline int sort_pairs(const SortBufs<P>& b, int64_t n, hipStream_t s, ErrorChannel& err) {
    const int64_t tiles = chunks(n), hist_len = tiles * kRadix;
    const unsigned grid = (unsigned)tiles;
    int rc;
    for (int pass = 0; pass < 4; ++pass) {
        const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
        eval_hist_kernel<<<grid, kThreads, 0, s>>>(b.keys[src], n, shift, b.hist, (int)tiles);
        if ((rc = err.launch_ok("eval_hist_kernel"))) return rc;
        if ((rc = scan_in_place(b.hist, hist_len, b.hist_sums, nullptr, s, err))) return rc;
        eval_scatter_kernel<P><<<grid, kThreads, 0, s>>>(b.keys[src], b.pay[src], b.keys[dst], b.pay[dst], n, shift, b.hist,
                                                         (int)tiles);
        if ((rc = err.launch_ok("eval_scatter_kernel"))) return rc;
    }
    return XVEC_OK;
}

}  // namespace
}  // namespace trial_sort
}  // namespace xvec
