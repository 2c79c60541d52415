"""What the tests of the scoring and evaluation back ends share: a restatement of gemm_nt's tile-size rule (csrc/score_tiles.h,
tests/test_score_tiles.py ties the two), the tile counts that follow from it, and a workspace window of an exact size inside
a guarded buffer.  A plain module like plda_em_ref.py; the test files import it."""
GUARD = 0xA5


def tile_count(M, N, sym, ts):
    """Tiles of edge ts the product computes: the symmetric walk visits only those on or above the diagonal."""
    tm, tn = -(-M // ts), -(-N // ts)
    return tm * (tm + 1) // 2 if sym else tm * tn


def gemm_tile_size(M, N, K, sym, pre, num_cu):
    """64 or 128: the prelude products always 64; otherwise 64 while 128 x 128 tiles would fill the 2 num_cu block slots less
    than one and a half times, or when the rounds of 64 x 64 tiles on 4 num_cu slots (a round weighs 0.49 of a 128 x 128 round
    at K <= 256, 0.53 beyond) cost less than the rounds of 128 x 128 tiles."""
    slots128, slots64 = 2 * num_cu, 4 * num_cu
    c128, c64 = tile_count(M, N, sym, 128), tile_count(M, N, sym, 64)
    r128, r64 = -(-c128 // slots128), -(-c64 // slots64)
    weight = 49 if K <= 256 else 53
    return 64 if pre or 2 * c128 < 3 * slots128 or r64 * weight < r128 * 100 else 128


def is_persistent(M, N, K, sym, num_cu):
    """Does a block of the score product (not a prelude) walk more than one tile?"""
    ts = gemm_tile_size(M, N, K, sym, False, num_cu)
    return tile_count(M, N, sym, ts) > (4 if ts == 64 else 2) * num_cu


def window(need, device):
    """(buffer, offset): `need` bytes of 0xFF (NaN as float64) at a 256-byte aligned offset inside a buffer of GUARD bytes."""
    import torch
    big = torch.full((need + 8192,), GUARD, dtype=torch.uint8, device=device)
    off = 4096 + (-(big.data_ptr() + 4096)) % 256
    assert (big.data_ptr() + off) % 256 == 0 and off + need <= big.numel() - 2048
    big[off:off + need] = 0xFF
    return big, off


def guards_intact(big, off, need):
    return bool((big[:off] == GUARD).all()) and bool((big[off + need:] == GUARD).all())
