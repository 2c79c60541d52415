// LDS image of one (product, plane) block of tdnn_wino_s3.hip: 64 pairs x 16 k bf16 = 2 KiB, a pair's 32 bytes in one row.
// Host-compilable (no HIP header, like mfcc_tables.h): tests/test_wino_s3_lds_map.py enumerates both maps below on the CPU.
//
// The plain image (row p at 32 p, k-byte kb at kb) is two-way bank-conflicted on both sides:
//   * ds_read_b128 is served in four groups of 16 lanes (lanes 0-3, 12-15, 20-27 | 4-11, 16-19, 28-31 | the same + 32), bank =
//     (a / 4) mod 64: a group must cover sixteen distinct 16-byte slots mod 256.  Its lanes share the k half h (lane >> 5) and
//     their rows take every value mod 8 exactly twice -- once with bit 3 of the row clear, once with it set.  So the 16-byte
//     piece of a row is swapped by bit 3 of the pair.
//   * ds_write_b64 is served in four groups of 16 consecutive lanes, bank = (a / 4) mod 32: a group must cover 128 distinct
//     bytes mod 128.  Sixteen consecutive threads stage four whole rows: pairs 2j, 2j + 1 (group 0) and 2j + 32, 2j + 33
//     (group 1), which the plain image puts 1 KiB apart -- the same 64 bytes mod 128.  So group 1's rows are swapped in twos
//     (row ^ 2): the four rows are then the four rows of one 128-byte line, mod 128.  (Swapping rows in twos permutes each
//     aligned set of four rows in itself, which leaves the read side's row-mod-8 argument as it is.)
#pragma once

namespace xvec {
namespace wino {

constexpr int kS3K = 16;                                  // k per chunk (one bf16 k-step)
constexpr int kS3Pairs = 64;                              // pairs of a tile (tdnn_wino_rows.h: kPairs)
constexpr int kS3Plane = kS3Pairs * kS3K * 2;             // bytes of one (product, plane) block: 64 pairs x 32 B
constexpr int kS3Stage = 4 * 3 * kS3Plane;                // one LDS buffer: 4 products x hi | mid | lo

// byte offset in a (product, plane) block of k-byte kb (0 .. 31) of pair p (0 .. 63) of the tile
constexpr int s3_lds_off(int p, int kb) {
    return (p ^ ((p >> 5) << 1)) * (kS3K * 2) + (((kb >> 4) ^ (p >> 3)) & 1) * 16 + (kb & 15);
}

// store side: thread tid stages 8 bytes (k 4 (tid & 3) .. + 3) of pair (tid >> 3) + 32 * ((tid >> 2) & 1)
constexpr int s3_st_off(int tid) { return s3_lds_off((tid >> 3) + 32 * ((tid >> 2) & 1), (tid & 3) * 8); }

// read side: lane (r = lane & 31, h = lane >> 5) reads the MFMA A fragment of pair r of pair group g: k 8h .. 8h + 7
constexpr int s3_a_rd(int lane, int g) { return s3_lds_off(32 * g + (lane & 31), 16 * (lane >> 5)); }

}  // namespace wino
}  // namespace xvec
