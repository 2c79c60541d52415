// The tile geometry of the fp64 score GEMM (csrc/score.hip): which tile a block walks next (tile_rc, tile_rc_sym) and which of
// the two tile sizes a product takes (gemm_tile_size).  Host-compilable (no HIP header, like mfcc_tables.h and dropout_mask.h):
// __device__ __forceinline__ under hipcc for the walks, plain inline C++ otherwise, so that tests/test_score_tiles.py can
// enumerate both walks and the rule on the CPU (tests/abi/score_tiles_dump.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XVEC_TILE_FN __device__ __forceinline__
#else
#define XVEC_TILE_FN inline
#endif

namespace xvec {
namespace score_tiles {

XVEC_TILE_FN int tile_min(int a, int b) { return a < b ? a : b; }

// Tile t of the walk -> (row tile, column tile).  The tiles are walked in 8 x 8 SUPERTILES (bands of eight row tiles, inside a
// band eight column tiles at a time, row-major inside the supertile): the 64 consecutive tiles an XCD's blocks work on at a time
// (xcd_remap) then share eight row operands and eight column operands -- 8 MiB at K = 512, the XCD's L2 twice over -- instead
// of two row operands and ALL column operands (row-major walk, round 4: 950 MB per 4874 x 4874 score matrix for 230 MB of
// operands and scores).  Bijective for any tiles_m x tiles_n (the last band / the last supertile of a band are narrower).
XVEC_TILE_FN void tile_rc(int t, int tiles_m, int tiles_n, int& r, int& c) {
    const int band = t / (8 * tiles_n);
    const int tb = t - band * 8 * tiles_n;
    const int h = tile_min(8, tiles_m - 8 * band);
    const int sc = tb / (8 * h);
    const int w = tile_min(8, tiles_n - 8 * sc);
    const int within = tb - sc * 8 * h;
    r = band * 8 + within / w;
    c = sc * 8 + within % w;
}

// The same walk over the tiles ON OR ABOVE the diagonal of a square tile grid (T x T, tile row <= tile column): band by band,
// the diagonal supertile first (its upper triangle row by row), then the band's other supertiles as above.  t < T (T + 1) / 2.
XVEC_TILE_FN void tile_rc_sym(int t, int T, int& r, int& c) {
    int band = 0;
    for (;;) {                                   // (T + 7) / 8 iterations at most, scalar
        const int h = tile_min(8, T - 8 * band);
        const int cnt = h * (h + 1) / 2 + h * (T - 8 * band - h);
        if (t < cnt) break;
        t -= cnt;
        ++band;
    }
    const int h = tile_min(8, T - 8 * band);
    int i = 0;
    for (; i < h; ++i) {                         // diagonal supertile: row i holds h - i tiles
        if (t < h - i) {
            r = band * 8 + i;
            c = band * 8 + i + t;
            return;
        }
        t -= h - i;
    }
    const int sc = t / (8 * h);                  // (h == 8 here: a shorter band is the last one and has no supertile to its right)
    const int w = tile_min(8, T - 8 * (band + 1 + sc));
    const int within = t - sc * 8 * h;
    r = band * 8 + within / w;
    c = (band + 1 + sc) * 8 + within % w;
}

// Tiles of edge `ts` a product of M x N scores has to compute (a symmetric walk visits only the tiles on or above the diagonal).
inline int64_t tile_count(int64_t M, int64_t N, bool sym, int64_t ts) {
    const int64_t tm = (M + ts - 1) / ts, tn = (N + ts - 1) / ts;
    return sym ? tm * (tm + 1) / 2 : tm * tn;
}

// The tile edge of one product, 64 or 128 (host only).  Two tilings:
//   128 x 128, two blocks per CU (255 registers);  64 x 64, FOUR blocks per CU (121 registers, 32 KiB of LDS each).
// Per CU the two finish the same work in the same time within a few per cent (a round of four 64 x 64 tiles against a round
// of two 128 x 128 ones: 0.49 for K <= 256, 0.53 for longer K, measured N = 1200 ... 16384, profiles/experiments/README.md), and
// a block slot walks ceil(tiles / slots) tiles -- so what decides is how full the LAST round is.  The reference's self-score
// of 4874 vectors is 780 tiles of 128 x 128 on 512 slots (two rounds, the second half empty) against 3003 of 64 x 64 on 1024
// (three rounds): 0.261 -> 0.200 ms in the low-rank form, 0.487 -> 0.411 dense (round 6; until then the 64 x 64 kernel ran two
// blocks per CU and served only products under a tile and a half per slot).
// (the prelude product stays on 64 x 64 tiles at every size: with the centring and the row dots on top, the 128 x 128 form
//  needs more registers than it has)
inline int gemm_tile_size(int64_t M, int64_t N, int K, bool sym, bool pre, int num_cu) {
    const int64_t slots128 = 2 * (int64_t)num_cu, slots64 = 4 * (int64_t)num_cu;      // persistent blocks per CU
    const int64_t c128 = tile_count(M, N, sym, 128), c64 = tile_count(M, N, sym, 64);
    const int64_t r128 = (c128 + slots128 - 1) / slots128, r64 = (c64 + slots64 - 1) / slots64;
    const bool small = pre || c128 * 2 < 3 * slots128 || r64 * (K <= 256 ? 49 : 53) < r128 * 100;
    return small ? 64 : 128;
}

}  // namespace score_tiles
}  // namespace xvec
