"""CPU-only checks of score normalisation (include/xvec_snorm.h): the longdouble reference against the definition written out
by brute force, the fp64 -> key map and the digit walk of csrc/snorm_keys.h through a dump program built with the host
compiler (tests/abi/snorm_keys_dump.cpp), the C ABI's argument errors (each returns before the library touches a device), and
the independence of the snorm error channel from the score and eval channels."""
import itertools
import math
import struct

import numpy as np
import pytest

import snorm_ref
from hipcc_support import header_constants, host_program, needs_host_cxx as needs_cxx
NAN = float("nan")
INF = float("inf")


# ---------------------------------------------------------------- the reference against the definition

def _brute(row, top_k, skip):
    """The definition, cell by cell: the valid cells, the k largest of them by repeated maximum, the sums as fractions."""
    from fractions import Fraction
    cells = [x for j, x in enumerate(row) if not math.isnan(x) and j != skip]
    k = len(cells) if top_k == 0 else min(top_k, len(cells))
    picked = []
    for _ in range(k):
        m = max(cells)
        cells.remove(m)
        picked.append(m)
    if k < 2:
        return k, NAN, NAN, NAN
    fr = [Fraction(x) for x in picked]
    mean = sum(fr) / k
    var = sum((x - mean) ** 2 for x in fr) / (k - 1)
    return k, min(picked), float(mean), math.sqrt(float(var))


ROWS = [
    ([3.0, 1.0, 2.0, 2.0, 2.0, 0.5], 3, -1),            # ties across the cut: two of the three 2.0 are taken
    ([3.0, 1.0, 2.0, 2.0, 2.0, 0.5], 0, -1),
    ([1.5, NAN, -2.0, 4.0, 0.25], 2, -1),               # a NaN cell
    ([1.5, NAN, -2.0, 4.0, 0.25], 0, -1),
    ([9.0, 1.0, 2.0, 3.0], 2, 0),                       # the maximum is the skipped column
    ([9.0, 1.0, 2.0, 3.0], 0, 3),
    ([1.0, 2.0, NAN, 3.0], 7, 1),                       # k clipped to v = 2
    ([NAN, 5.0, NAN], 2, -1),                           # one valid cell: NaN outputs, n_used 1
    ([NAN, NAN], 0, -1),
    ([-1.0, -3.0, -2.0, -2.0], 3, -1),
]


def test_reference_equals_the_definition_written_out():
    for row, top_k, skip in ROWS:
        ref = snorm_ref.row_stats(np.array([row]), top_k, None if skip < 0 else [skip])
        k, kth, mean, std = _brute(row, top_k, skip)
        assert ref.n_used[0] == k, (row, top_k, skip)
        if k < 2:
            assert np.isnan(ref.kth[0]) and np.isnan(ref.mean[0]) and np.isnan(ref.std[0])
            continue
        assert float(ref.kth[0]) == kth, (row, top_k, skip)
        assert abs(float(ref.mean[0]) - mean) <= 4 * snorm_ref.U * abs(mean), (row, top_k, skip)
        assert abs(float(ref.std[0]) - std) <= 4 * snorm_ref.U * std, (row, top_k, skip)
    # -1 in skip_col skips nothing, and the cut inside a run of ties does not depend on which of them is taken
    a = snorm_ref.row_stats(np.array([[2.0, 2.0, 2.0, 1.0]]), 2, [-1])
    assert a.n_used[0] == 2 and float(a.kth[0]) == 2.0 and float(a.mean[0]) == 2.0 and float(a.std[0]) == 0.0
    z = snorm_ref.row_stats(np.array([[-0.0, 0.0, -1.0]]), 2)
    assert float(z.kth[0]) == 0.0 and not np.signbit(np.float64(z.kth[0]))


def test_reference_apply_is_the_formula():
    s = np.array([[1.0, 2.0, 4.0], [0.5, -1.0, 3.0]])
    row, col = (np.array([1.0, 0.0]), np.array([2.0, 4.0])), (np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 0.5]))
    z, t, sn = snorm_ref.apply(s, row=row), snorm_ref.apply(s, col=col), snorm_ref.apply(s, row, col)
    assert float(z[1, 2]) == (3.0 - 0.0) / 4.0 and float(t[0, 2]) == (4.0 - 2.0) / 0.5
    assert float(sn[0, 1]) == 0.5 * (2.0 - 1.0) / 2.0 + 0.5 * (2.0 - 1.0) / 2.0


# ---------------------------------------------------------------- the key map and the digit walk

def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return host_program("snorm_keys_dump", tmp_path_factory.mktemp("snorm_keys"))


def _ordered_doubles():
    """Ascending, every neighbour pair either one ulp apart or far apart; -0.0 directly in front of +0.0."""
    tiny, dmax = 5e-324, 1.7976931348623157e308
    pos = [tiny, 2 * tiny, 2.2250738585072009e-308, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 1.0),
           1e-300, np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 1.5, 2.0, 1e6, np.nextafter(1e6, 2e6), 1e300,
           np.nextafter(dmax, 0.0), dmax]
    pos = [float(x) for x in pos]
    return [-INF] + [-x for x in reversed(pos)] + [-0.0, 0.0] + pos + [INF]


@needs_cxx
def test_key_map_is_monotone_exact_and_classifies_nans(dump):
    xs = _ordered_doubles()
    assert all(a < b or (a == 0.0 and b == 0.0) for a, b in zip(xs, xs[1:]))
    lines = dump([f"key {_bits(x):016x}" for x in xs])
    keys, back = [], []
    for x, line in zip(xs, lines):
        _, nan, key, value_bits = line.split()
        assert nan == "0", x
        keys.append(int(key, 16))
        back.append(int(value_bits, 16))
    for (a, ka), (b, kb) in zip(zip(xs, keys), zip(xs[1:], keys[1:])):
        assert (ka < kb) == (a < b) and (ka == kb) == (a == b), (a, b)
    z = xs.index(0.0)                                                                    # -0.0 (it equals 0.0); +0.0 follows
    assert np.signbit(xs[z]) and not np.signbit(xs[z + 1]) and keys[z] == keys[z + 1] == 0x8000000000000000
    assert min(keys) == 0x000fffffffffffff > 0                                           # -inf: above the void key 0
    for x, u in zip(xs, back):                                                           # the round trip is exact
        assert u == (_bits(0.0) if x == 0.0 else _bits(x)), x
    nans = [0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001, 0x7fffffffffffffff,
            0xffffffffffffffff, _bits(NAN)]
    for u, line in zip(nans, dump([f"key {u:016x}" for u in nans])):
        assert line.split()[1] == "1", hex(u)
    for u in (_bits(INF), _bits(-INF), _bits(1.7976931348623157e308)):                   # the neighbours of the NaN class
        assert dump([f"key {u:016x}"])[0].split()[1] == "0"


@needs_cxx
def test_digit_walk_finds_the_kth_largest_key(dump):
    rng = np.random.default_rng(7)
    key = 0x0123456789abcdef
    assert dump([f"digits {key:016x}"])[0].split()[1:] == [str(b) for b in key.to_bytes(8, "big")]
    rows = [rng.standard_normal(37), np.full(9, 2.5), np.array([1.0, 1.0, 3.0, 3.0, 3.0, -2.0]),
            np.array([-0.0, 0.0, -1.0, 0.0]), np.array([INF, -INF, 1.0, NAN, 2.0]), 1e6 + rng.standard_normal(50),
            np.array([5e-324, -5e-324, 0.0, 1e-310])]
    requests, want = [], []
    for row in rows:
        valid = np.sort(row[~np.isnan(row)])[::-1]
        for k in range(1, valid.size + 1):
            requests.append(f"select {k} {row.size} " + " ".join(f"{_bits(float(x)):016x}" for x in row))
            want.append((float(valid[k - 1]), int((valid > valid[k - 1]).sum())))
    kth_keys = [int(line.split()[2], 16) for line in dump([f"key {_bits(kth):016x}" for kth, _ in want])]
    for line, (kth, above), kth_key in zip(dump(requests), want, kth_keys):
        _, cut, n_above = line.split()
        assert int(cut, 16) == kth_key, (line, kth)
        assert int(n_above) == above, line


# ---------------------------------------------------------------- the C ABI without a device

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first


def _row_stats(lib, scores=P, ld=8, n=4, C=8, top_k=0, skip=None, mean=P, std=P, kth=P, n_used=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.xvec_snorm_workspace_bytes(n, C)
    return lib.xvec_snorm_row_stats(scores, ld, n, C, top_k, skip, mean, std, kth, n_used, ws, ws_bytes, None)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_snorm_last_error().decode()
    need = lib.xvec_snorm_workspace_bytes(4, 8)
    assert need >= 4 * 16 and need % 256 == 0
    cases = [
        (dict(n=0), hip.ERR_ARG, "n = 0: need at least one row"),
        (dict(n=-3), hip.ERR_ARG, "n = -3: need at least one row"),
        (dict(C=0, ld=0), hip.ERR_ARG, "C = 0: need at least one cohort column"),
        (dict(C=-1, ld=0), hip.ERR_ARG, "C = -1: need at least one cohort column"),
        (dict(ld=7), hip.ERR_ARG, "ld = 7 is smaller than C = 8"),
        (dict(top_k=-1), hip.ERR_ARG, "top_k = -1 must not be negative (0 = every valid cell)"),
        (dict(scores=None), hip.ERR_ARG, "null pointer: scores"),
        (dict(mean=None), hip.ERR_ARG, "null pointer: mean / std / kth / n_used"),
        (dict(std=None), hip.ERR_ARG, "null pointer: mean / std / kth / n_used"),
        (dict(kth=None), hip.ERR_ARG, "null pointer: mean / std / kth / n_used"),
        (dict(n_used=None), hip.ERR_ARG, "null pointer: mean / std / kth / n_used"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
        (dict(n=2 ** 31, ws_bytes=1 << 40), hip.ERR_TOO_LARGE, f"cohort score matrix [{2 ** 31}, 8]: both sizes must be at most 2^31 - 1"),
    ]
    for kwargs, code, text in cases:
        assert _row_stats(lib, **kwargs) == code, kwargs
        assert err() == text, kwargs
    for n, C in ((0, 8), (8, 0), (-1, 8), (8, -1), (2 ** 31, 8), (8, 2 ** 31)):
        assert lib.xvec_snorm_workspace_bytes(n, C) == 0, (n, C)
    assert lib.xvec_snorm_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 0

    apply = lambda **kw: lib.xvec_snorm_apply(*[{**dict(scores=P, ld=8, n_rows=4, n_cols=8, rm=P, rs=P, cm=P, cs=P, out=P + 0x10000,
                                                        ld_out=8, stream=None), **kw}[a]
                                                for a in ("scores", "ld", "n_rows", "n_cols", "rm", "rs", "cm", "cs", "out", "ld_out", "stream")])
    cases = [
        (dict(rm=None, rs=None, cm=None, cs=None), "neither row nor column statistics: nothing to normalise with"),
        (dict(rm=None), "a mean and its std must both be given or both be null"),
        (dict(cs=None), "a mean and its std must both be given or both be null"),
        (dict(n_rows=0), "score matrix [0, 8]: both sizes must be in 1 .. 2^31 - 1"),
        (dict(n_cols=0, ld=0), "score matrix [4, 0]: both sizes must be in 1 .. 2^31 - 1"),
        (dict(ld=7), "ld = 7 and ld_out = 8 must be at least n_cols = 8"),
        (dict(ld_out=7), "ld = 8 and ld_out = 7 must be at least n_cols = 8"),
        (dict(scores=None), "null pointer: scores / out"),
        (dict(out=None), "null pointer: scores / out"),
        (dict(out=P, ld_out=9), "in place (out == scores) needs ld_out == ld (got 9 and 8)"),
    ]
    for kwargs, text in cases:
        assert apply(**kwargs) == hip.ERR_ARG, kwargs
        assert err() == text, kwargs


def test_snorm_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    score = (lambda: lib.xvec_gemm_nt_f64(None, 0, None, 0, -1, 0, 1, None, None, 0.0, 1.0, None, 0, None),
             lib.xvec_score_last_error, "bad GEMM shape M=-1 N=0 K=1")
    evalc = (lambda: lib.xvec_eval_trials(None, 0, 0, 0, None, None, None, 0, 1.0, 1.0, 0.5, None, None, 0, None),
             lib.xvec_eval_last_error, "n_trials = 0: need at least one trial")
    snorm = (lambda: _row_stats(lib, top_k=-5), lib.xvec_snorm_last_error, "top_k = -5 must not be negative (0 = every valid cell)")
    for order in itertools.permutations((score, evalc, snorm)):
        raised = []
        for provoke, last_error, want in order:
            assert provoke() == hip.ERR_ARG
            raised.append((last_error, want))
            for le, w in raised:                  # its own message, and the channels that failed before still hold theirs
                assert le().decode() == w
    # a failing snorm call of another kind changes the snorm text only
    assert _row_stats(lib, ld=1) == hip.ERR_ARG
    assert lib.xvec_snorm_last_error().decode() == "ld = 1 is smaller than C = 8"
    assert lib.xvec_score_last_error().decode() == score[2] and lib.xvec_eval_last_error().decode() == evalc[2]


def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import re
    import torch
    from xvector_amd import snorm
    consts = header_constants("xvec_snorm.h", "XVEC_SNORM_")
    assert consts == {"THREADS": snorm.THREADS, "RESIDENT_SMALL": snorm.RESIDENT_SMALL, "RESIDENT_MAX": snorm.RESIDENT_MAX,
                      "APPLY_ROWS": snorm.APPLY_ROWS, "APPLY_COLS": snorm.APPLY_COLS}
    with pytest.raises(RuntimeError, match="HIP device only"):
        snorm.cohort_stats(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device only"):
        snorm.apply_norm(torch.zeros(3, 4, dtype=torch.float64), row_stats=(torch.zeros(3), torch.ones(3)))
    with pytest.raises(RuntimeError, match="HIP device only"):
        snorm.ScoreNormalizer("cosine", np.zeros((4, 8)), device="cpu")
