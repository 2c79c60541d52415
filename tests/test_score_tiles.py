"""The tile geometry of the fp64 score GEMM (csrc/score_tiles.h) on the CPU: tests/abi/score_tiles_dump.cpp, compiled with the
host compiler, walks tile_rc and tile_rc_sym over whole grids and answers the tile-size rule; the test checks that both walks
visit every tile exactly once, that a supertile of the plain walk is what the L2 sharing rests on, and that the restatement of
the rule the GPU tests plan their shapes with (tests/score_support.py) is the header's.  No GPU, no HIP library."""
import numpy as np
import pytest

import score_support as ss
from hipcc_support import host_program, needs_host_cxx

pytestmark = needs_host_cxx

THIN = [(1, 300), (300, 1), (9, 77), (77, 9), (8, 129), (129, 8), (17, 64)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return host_program("score_tiles_dump", tmp_path_factory.mktemp("score_tiles"))


def _pairs(line, head):
    v = np.array(line.split()[head:], dtype=np.int64)
    return v[0::2], v[1::2]


@pytest.fixture(scope="module")
def plain_walks(dump):
    grids = [(m, n) for m in range(1, 41) for n in range(1, 41)] + THIN
    return {g: _pairs(line, 3) for g, line in zip(grids, dump([f"rc {m} {n}" for m, n in grids]))}


def test_plain_walk_visits_every_tile_once(plain_walks):
    for (tm, tn), (r, c) in plain_walks.items():
        assert r.size == tm * tn
        assert r.min() >= 0 and r.max() < tm and c.min() >= 0 and c.max() < tn, (tm, tn)
        assert np.unique(r * tn + c).size == tm * tn, f"{tm} x {tn}: a tile is visited twice"


def test_symmetric_walk_visits_every_tile_of_the_upper_triangle_once(dump):
    Ts = list(range(1, 131))
    for T, line in zip(Ts, dump([f"sym {T}" for T in Ts])):
        r, c = _pairs(line, 2)
        assert r.size == T * (T + 1) // 2
        assert r.min() >= 0 and c.max() < T and (r <= c).all(), f"T = {T}: a tile outside the upper triangle"
        assert np.unique(r * T + c).size == r.size, f"T = {T}: a tile is visited twice"
        diag = np.flatnonzero(r == c)
        # the diagonal supertile comes first in its band: the band's first tile is its diagonal tile
        first_of_band = [int(np.flatnonzero(r // 8 == b)[0]) for b in range((T + 7) // 8)]
        assert all(r[t] == c[t] == 8 * b for b, t in enumerate(first_of_band)), T
        assert diag.size == T


def test_a_supertile_shares_eight_row_and_eight_column_operands(plain_walks):
    """What the XCD remap rests on: inside a full band (eight row tiles) the 64 consecutive tiles that start at a multiple of
    64 from the band's first tile are one supertile: at most 8 row tiles and 8 column tiles.  Where the bands themselves start
    at multiples of 64 (tiles_n a multiple of 8) that holds for every aligned group of 64 tiles of the whole walk."""
    checked = 0
    for (tm, tn), (r, c) in plain_walks.items():
        for band in range(tm // 8):                      # the full bands
            t0 = band * 8 * tn
            for g0 in range(t0, t0 + 8 * tn, 64):
                g1 = min(g0 + 64, t0 + 8 * tn)
                assert np.unique(r[g0:g1]).size <= 8 and np.unique(c[g0:g1]).size <= 8, (tm, tn, g0)
                assert (r[g0:g1] // 8 == band).all()
                checked += 1
        if tn % 8 == 0:
            for g0 in range(0, (tm // 8) * 8 * tn, 64):
                assert np.unique(r[g0:g0 + 64]).size <= 8 and np.unique(c[g0:g0 + 64]).size <= 8, (tm, tn, g0)
    assert checked > 1000


def test_tile_size_rule_equals_its_restatement(dump):
    sizes = [1, 63, 64, 65, 128, 129, 449, 1024, 1089, 2817, 3500, 3601, 4874, 5600, 5700, 6143, 6144, 6145, 8192]
    cases = [(M, N, K, sym, pre, cu) for M in sizes for N in sizes for K in (16, 256, 257, 512) for sym in (0, 1)
             for pre in (0, 1) for cu in (64, 256, 304) if not sym or M == N]
    got = [int(line.split()[1]) for line in dump([f"rule {M} {N} {K} {s} {p} {cu}" for M, N, K, s, p, cu in cases])]
    want = [ss.gemm_tile_size(M, N, K, bool(s), bool(p), cu) for M, N, K, s, p, cu in cases]
    assert got == want
    assert set(got) == {64, 128}
    assert all(g == 64 for g, case in zip(got, cases) if case[4]), "a prelude product on 128 x 128 tiles"
    # the shapes the README and tests/test_scoring.py quote, on the 256 CUs of an MI355X
    assert ss.gemm_tile_size(4874, 4874, 512, True, False, 256) == 64
    assert ss.gemm_tile_size(5600, 5600, 512, True, False, 256) == 128
    assert ss.gemm_tile_size(5600, 5600, 200, True, False, 256) == 64
    assert ss.gemm_tile_size(3601, 3500, 272, False, False, 256) == 128
    assert ss.gemm_tile_size(3601, 3500, 48, False, False, 256) == 64
