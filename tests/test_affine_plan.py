"""The dispatch arithmetic of the segment-layer GEMMs (csrc/affine_plan.h) on the CPU: tests/abi/affine_plan_dump.cpp, compiled
with the host compiler, answers the plan of a list of shapes; the test checks the properties the kernels of csrc/affine.hip
rest on over a seeded sweep, and pins the plans of the shapes the GPU tests (tests/test_affine_forms_gpu.py) and the benchmark
run -- a change to one of them must be deliberate.  No GPU, no HIP library."""
import numpy as np
import pytest

from hipcc_support import host_program, needs_host_cxx

pytestmark = needs_host_cxx

TILE16, TILE16_ELEM, SPLITK, SPLITK_X3, DIRECT, DIRECT_X3 = 1, 2, 3, 4, 5, 6      # affine_plan::Form
MAX_SEGMENTS = 65535 * 16        # what xvec_forward_segments accepts per call (include/xvec_hip.h)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    ask = host_program("affine_plan_dump", tmp_path_factory.mktemp("affine_plan"))

    def plans(cases):
        """cases: (M, N, K, vec16_ok, out_ok, scratch_floats, have_w3) -> dicts"""
        out = []
        for c, line in zip(cases, ask([" ".join(str(int(v)) for v in c) for c in cases])):
            v = [int(t) for t in line.split()]
            d = dict(zip(("form", "S", "tps", "s_pad", "grid_x", "grid_y", "trips"), v[:7]))
            d["ranges"] = list(zip(v[7::2], v[8::2]))
            d["case"] = c
            out.append(d)
        return out
    return plans


def ample(M, N):
    return 20 * M * N


def test_properties_over_a_seeded_sweep(dump):
    rng = np.random.default_rng(20240611)
    n = 2000
    M = rng.integers(1, 20001, n)
    M[::2] = np.exp(rng.uniform(0, np.log(20000), len(M[::2]))).astype(np.int64)      # half of them log-uniform: few tiles
    N = rng.integers(4, 2049, n)
    N[: n // 2] = (N[: n // 2] + 3) // 4 * 4                 # half the sweep on widths the 64 x 64 forms accept
    K = rng.integers(4, 4097, n)
    K[: 3 * n // 4] = (K[: 3 * n // 4] + 3) // 4 * 4
    frac = rng.uniform(0, 20, n)
    frac[::7] = rng.integers(0, 21, len(frac[::7]))          # exact multiples of M N: the edge of "holds S partials"
    scratch = np.floor(frac * M * N).astype(np.int64)
    cases = [(m, nn, k, k % 4 == 0 and i % 11 != 0, i % 13 != 0, s, i % 2) for i, (m, nn, k, s) in enumerate(zip(M, N, K, scratch))]
    # the extremes of what xvec_forward_segments accepts, at the model widths
    cases += [(m, nn, k, 1, 1, s * m * nn, w) for m in (MAX_SEGMENTS, MAX_SEGMENTS - 15, 65536 * 8) for nn, k in ((512, 3000), (512, 512), (1211, 512), (8, 8))
              for s in (0, 1, 20) for w in (0, 1)]
    seen = set()
    for p in dump(cases):
        m, nn, k, vec, ok, s, w3 = p["case"]
        what = f"M={m} N={nn} K={k} vec16={vec} out_ok={ok} scratch={s} w3={w3}: {p}"
        seen.add((p["form"], p["S"]))
        assert p["trips"] == -(-k // 64)
        # the ranges tile [0, trips) exactly: no gap, no overlap, no empty range
        assert len(p["ranges"]) == p["S"] >= 1, what
        assert p["ranges"][0][0] == 0 and p["ranges"][-1][1] == p["trips"], what
        assert all(lo < hi for lo, hi in p["ranges"]), what
        assert all(a[1] == b[0] for a, b in zip(p["ranges"], p["ranges"][1:])), what
        assert 0 < p["grid_x"] <= 2 ** 31 - 1 and 0 < p["grid_y"] <= 65535, what
        if p["S"] > 1:
            assert p["form"] in (SPLITK, SPLITK_X3), what
            assert p["tps"] >= 2 and p["S"] <= 16, what
            assert p["S"] * m * nn <= s, what
            assert p["s_pad"] % 8 == 0 and p["s_pad"] >= p["S"], what
            assert p["grid_x"] == p["s_pad"] * -(-m // 64) * -(-nn // 64), what
        else:
            assert p["form"] in (TILE16, TILE16_ELEM, DIRECT, DIRECT_X3) and p["tps"] == p["trips"], what
        if p["form"] in (TILE16, TILE16_ELEM):
            assert (p["grid_x"], p["grid_y"]) == (-(-nn // 16), -(-m // 16)), what
            assert (p["form"] == TILE16) == bool(vec), what
        else:                                                # the 64 x 64 forms: what their loads and stores assume
            assert vec and ok and nn % 4 == 0 and k % 4 == 0, what
            assert (p["form"] in (SPLITK_X3, DIRECT_X3)) == bool(w3), what
        if p["form"] in (DIRECT, DIRECT_X3):
            assert p["grid_x"] == -(-m // 64) * -(-nn // 64) >= 256 and p["grid_y"] == 1, what
    assert {f for f, _ in seen} == {TILE16, TILE16_ELEM, SPLITK, SPLITK_X3, DIRECT, DIRECT_X3}
    assert {s for _, s in seen} >= {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16}, sorted(seen)


def _one(dump, M, N, K, scratch, w3=0, vec=1, ok=1):
    return dump([(M, N, K, vec, ok, scratch, w3)])[0]


L6 = (512, 3000)
PINNED_S = [  # (N, K), M, scratch in units of M N (None: ample), S
    (L6, 1, None, 16), (L6, 63, None, 16), (L6, 65, None, 16), (L6, 256, None, 16), (L6, 257, None, 12), (L6, 448, None, 10),
    (L6, 449, None, 8), (L6, 641, None, 6), (L6, 1025, None, 4), (L6, 2049, None, 2), (L6, 4032, None, 2),
    (L6, 500, 2, 2), (L6, 500, 3, 3), (L6, 500, 5, 5), (L6, 500, 7, 7),
    ((448, 448), 37, None, 3), ((512, 512), 37, None, 4), ((200, 200), 37, None, 2), ((252, 252), 37, None, 2),
    ((1212, 512), 37, None, 4), ((60, 448), 37, None, 3),
    ((512, 512), 256, None, 4),                              # the benchmark batch: layer 7 (layer 6 is (L6, 256) above)
]
PINNED_TILE16 = [(L6, 500, 1.999), (L6, 500, 1), (L6, 500, 0), (L6, 1984, 1.999), (L6, 1984, 0),
                 ((64, 64), 37, None), ((128, 128), 37, None), ((192, 192), 37, None), ((1211, 512), 37, None),
                 ((1211, 512), 256, None),                   # the benchmark batch: output
                 ((64, 64), 16320, None), ((64, 64), 16320, 0), ((64, 64), 16320, 1)]
PINNED_DIRECT = [(L6, 4033, None), (L6, 1985, 1.999), (L6, 1985, 0), ((64, 64), 16321, None), ((64, 64), 16321, 0),
                 ((64, 64), 16321, 1)]


def _scratch(M, N, units):
    return ample(M, N) if units is None else int(units * M * N)


@pytest.mark.parametrize("w3", [0, 1])
def test_pinned_plans(dump, w3):
    for (N, K), M, units, S in PINNED_S:
        p = _one(dump, M, N, K, _scratch(M, N, units), w3)
        assert (p["form"], p["S"]) == (SPLITK_X3 if w3 else SPLITK, S), (N, K, M, units, p)
    for (N, K), M, units in PINNED_TILE16:
        p = _one(dump, M, N, K, _scratch(M, N, units), w3)
        assert (p["form"], p["S"]) == (TILE16, 1), (N, K, M, units, p)
    for (N, K), M, units in PINNED_DIRECT:
        p = _one(dump, M, N, K, _scratch(M, N, units), w3)
        assert (p["form"], p["S"]) == (DIRECT_X3 if w3 else DIRECT, 1), (N, K, M, units, p)
    # the ranges themselves where the GPU tests count on them
    p = _one(dump, 256, 512, 3000, ample(256, 512), w3)
    assert p["tps"] == 3 and p["ranges"][-1] == (45, 47) and p["s_pad"] == 16 and p["grid_x"] == 16 * 4 * 8
    p = _one(dump, 37, 448, 448, ample(37, 448), w3)
    assert p["tps"] == 3 and p["ranges"] == [(0, 3), (3, 6), (6, 7)] and p["s_pad"] == 8      # the last range: one trip
    p = _one(dump, 37, 512, 512, ample(37, 512), w3)
    assert p["tps"] == 2 and p["ranges"] == [(0, 2), (2, 4), (4, 6), (6, 8)]
    p = _one(dump, 16321, 64, 64, 0, w3)
    assert p["trips"] == p["tps"] == 1 and p["grid_x"] == 256
    p = _one(dump, 1984, 512, 3000, 1984 * 512, w3)
    assert (p["grid_x"], p["grid_y"]) == (32, 124)           # 31 x 8 = 248 tiles of 64 x 64: under the direct form's 256
    # the last ranges of layer 6's plans: 2, 3, 5, 7, 11, 15 and 23 trips (both register sets, odd and even counts)
    last = {}
    for M, units in ((256, None), (257, None), (448, None), (449, None), (641, None), (1025, None), (2049, None), (500, 3),
                     (500, 5), (500, 7)):
        p = _one(dump, M, 512, 3000, _scratch(M, 512, units), w3)
        last[p["S"]] = p["ranges"][-1][1] - p["ranges"][-1][0]
    assert last == {16: 2, 12: 3, 10: 2, 8: 5, 6: 7, 4: 11, 2: 23, 3: 15, 5: 7, 7: 5}, last


def test_what_keeps_the_64x64_forms_away(dump):
    """No scratch offered (xvec_affine), an output or bias off 16 bytes: tile16 whatever the shape; operands off 16 bytes or
    K % 4 != 0: the element-wise tile16 kernel; N % 4 != 0: tile16."""
    for M in (37, 256, 4033):
        assert _one(dump, M, 512, 3000, ample(M, 512), ok=0)["form"] == TILE16
        assert _one(dump, M, 512, 3000, ample(M, 512), vec=0)["form"] == TILE16_ELEM
        assert _one(dump, M, 512, 3000, ample(M, 512), vec=0, ok=0)["form"] == TILE16_ELEM
        assert _one(dump, M, 510, 3000, ample(M, 510))["form"] == TILE16
    assert _one(dump, 37, 66, 66, ample(37, 66), vec=0, w3=0)["form"] == TILE16_ELEM
