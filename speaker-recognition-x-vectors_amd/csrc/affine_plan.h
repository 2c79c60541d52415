// Which kernel form a segment-layer GEMM y[M,N] = act(x[M,K] . W[N,K]^T + b) takes (csrc/affine.hip), and with which K
// ranges and grid.  Host arithmetic only and host-compilable (no HIP header, like score_tiles.h, snorm_keys.h and
// resample_taps.h), so that tests/test_affine_plan.py can check the plan on the CPU (tests/abi/affine_plan_dump.cpp).
// launch_affine_f32 launches what plan() returns and decides nothing itself.
#pragma once
#include <cstdint>

namespace xvec {
namespace affine_plan {

// the values of XVEC_AFFINE_* (include/xvec_hip.h; csrc/xvec_api.hip asserts that they are)
enum Form {
    kNone = 0,
    kTile16 = 1,         // affine_f32_kernel<true>: one 16 x 16 tile per block, 16-byte loads
    kTile16Elem = 2,     // affine_f32_kernel<false>: the same, element-wise loads (K % 4 != 0 or a base off 16 bytes)
    kSplitK = 3,         // affine_splitk_kernel<false> + affine_reduce_kernel: 64 x 64 tiles x S ranges of K, fp32 MFMAs
    kSplitKX3 = 4,       // affine_splitk_x3_kernel (S > 1) + affine_reduce_kernel: the same on bf16x3 products
    kDirect = 5,         // affine_splitk_kernel<true>: 64 x 64 tiles over the whole K, written to y
    kDirectX3 = 6        // affine_splitk_x3_kernel with S == 1
};

constexpr int kTripK = 64;        // k of one trip of the 64 x 64 forms (one staged operand tile)
constexpr int kMaxRanges = 16;    // affine_reduce_kernel requests that many partials at once
constexpr int kFillBlocks = 512;  // the split aims at this many blocks: about two per CU
constexpr int kDirectTiles = 256; // from this many 64 x 64 tiles on the tiles alone fill the chip

struct Plan {
    int form;              // Form
    int S;                 // K ranges (1: no split -- the direct and tile16 forms)
    int trips_per_range;   // trips of 64 k per range; range s covers trips [s * trips_per_range, min(trips, (s + 1) * trips_per_range))
    int s_pad;             // split-K forms: S rounded up to the eight XCDs, the ranges S .. s_pad - 1 are blocks that exit at once; else 0
    int64_t grid_x, grid_y;
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// vec16_ok: K % 4 == 0 and x and W are 16-byte aligned (the 16-byte loads of every form but kTile16Elem).
// out_ok:   the caller offers scratch (a window of 0 floats still counts) and y and b are 16-byte aligned: the 64 x 64
//           forms may be taken (they also need N % 4 == 0: affine_reduce_kernel writes a float4 of y per thread).
// scratch_floats: what the split-K partials [S][M][N] may take.
// have_w3:  W is also there as bf16 pairs (launch_split_pairs): the 64 x 64 forms run on bf16x3 products.
inline Plan plan(int M, int N, int K, bool vec16_ok, bool out_ok, int64_t scratch_floats, bool have_w3) {
    Plan p;
    const int64_t MN = (int64_t)M * N;
    const int64_t tm = ceil_div(M, 64), tn = ceil_div(N, 64), trips = ceil_div(K, kTripK);
    if (out_ok && vec16_ok && N % 4 == 0 && MN > 0) {
        int64_t S = ceil_div(kFillBlocks, tm * tn);                                  // about two blocks per CU
        S = min64(S, trips / 2 > 1 ? trips / 2 : 1);                                 // at least two trips per range
        S = min64(S, kMaxRanges);
        S = min64(S, (scratch_floats > 0 ? scratch_floats : 0) / MN);                // as many partials as the scratch holds
        if (S <= 1 && tm * tn >= kDirectTiles) {
            p.form = have_w3 ? kDirectX3 : kDirect;
            p.S = 1;
            p.trips_per_range = (int)trips;
            p.s_pad = 0;
            p.grid_x = tn * tm;
            p.grid_y = 1;
            return p;
        }
        if (S > 1) {
            const int64_t tps = ceil_div(trips, S);
            S = ceil_div(trips, tps);                                                // no empty range
            p.form = have_w3 ? kSplitKX3 : kSplitK;
            p.S = (int)S;
            p.trips_per_range = (int)tps;
            p.s_pad = (int)((S + 7) & ~(int64_t)7);
            p.grid_x = p.s_pad * tn * tm;
            p.grid_y = 1;
            return p;
        }
    }
    p.form = vec16_ok ? kTile16 : kTile16Elem;
    p.S = 1;
    p.trips_per_range = (int)trips;
    p.s_pad = 0;
    p.grid_x = ceil_div(N, 16);
    p.grid_y = ceil_div(M, 16);
    return p;
}

}  // namespace affine_plan
}  // namespace xvec
