"""CPU-only checks of resampling (include/xvec_resample.h): the tap plan of csrc/resample_taps.h through a dump program built
with the host compiler (tests/abi/resample_taps_dump.cpp) against the numpy restatement (tests/resample_ref.py), bit for bit;
the restatement's vectorised form against its literal double loop; the filter table against its formula; the restatement
against an analytic sine (a check that does not come from the same formula); the C ABI's argument errors (each returns before the
library touches a device) and its error channel; the Python module's constants and its refusal of the CPU."""
import struct

import numpy as np
import pytest

import resample_ref as ref
from hipcc_support import header_constants, host_program, needs_host_cxx as needs_cxx

RATIOS = [2.0, 1.0, 16000 / 48000, 16000 / 44100, 44100 / 16000, 16000 / 22050, 16000 / 11025, 1 / 0.9, 1 / 1.1]
PRECISION = 9
NWIN = 64 * 512 + 1


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.fixture(scope="module")
def best():
    return ref.sinc_window(**ref.KAISER_BEST)


# ---------------------------------------------------------------- the tap plan

@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    program = host_program("resample_taps_dump", tmp_path_factory.mktemp("resample_taps"), "-ffp-contract=off")
    return lambda requests: program.output(stdin="\n".join(requests) + "\n").splitlines()      # (a request has many answer lines)


def _check_taps(lines, jobs):
    """`jobs`: (t0, t1, ratio, n) in request order; every line of the dump against ref.tap_plan, eta as bit patterns."""
    it = iter(lines)
    for t0, t1, ratio, n in jobs:
        for t in range(t0, t1):
            f = next(it).split()
            n0, off_l, eta_l, i_max, off_r, eta_r, k_max = ref.tap_plan(t, ratio, PRECISION, NWIN, n)
            got = (int(f[1]), int(f[2]), int(f[3]), int(f[4], 16), int(f[5]), int(f[6]), int(f[7]), int(f[8], 16), int(f[9]))
            want = (t, n0, off_l, _bits(eta_l), 0, i_max, off_r, _bits(eta_r), max(k_max, 0))
            assert f[0] == "tap" and got == want, (ratio, n, t, got, want)
            assert n0 < n and 0 <= eta_l < 1 and 0 <= eta_r < 1, (ratio, n, t)
    assert next(it, None) is None


@needs_cxx
def test_ratio_plan_and_output_length_are_the_reference_s(dump):
    lines = dump([f"ratio {_bits(r):016x} {PRECISION}" for r in RATIOS])
    for r, line in zip(RATIOS, lines):
        inc, scale, step = ref.ratio_plan(r, PRECISION)
        assert line.split() == ["ratio", f"{_bits(inc):016x}", f"{_bits(scale):016x}", str(step), str(int(r < 1))], r
    assert ref.ratio_plan(16000 / 48000, PRECISION)[2] == 170           # 512 / 3, truncated: the package's behaviour, kept
    sizes = list(range(0, 200)) + [3000, 3001, 44100, 48000, 2 ** 31 - 1]
    reqs = [(n, r) for r in RATIOS for n in sizes]
    for (n, r), line in zip(reqs, dump([f"len {n} {_bits(r):016x}" for n, r in reqs])):
        assert line.split() == ["len", str(ref.num_out(n, r))], (n, r)
    # the input span of a tile: its centres plus both wings
    for r, line in zip(RATIOS, dump([f"span {_bits(r):016x} {PRECISION} {NWIN} 256" for r in RATIOS])):
        inc, _, step = ref.ratio_plan(r, PRECISION)
        assert int(line.split()[1]) == int(255 * inc) + 1 + 2 * (NWIN // step), r


@needs_cxx
def test_tap_plan_equals_the_reference_for_every_output(dump):
    """Every t of rows of a few thousand samples, of rows shorter than one wing, and of rows with no or one output."""
    jobs = []
    for r in RATIOS:
        sizes = [1, 2, 63, 64, 65, 191, 192, 193, 1000, 3001]
        sizes += [n for n in range(1, 12) if ref.num_out(n, r) in (0, 1)]
        jobs += [(0, ref.num_out(n, r), r, n) for n in sizes]
    assert any(j[1] == 0 for j in jobs) and any(j[1] == 1 for j in jobs)
    lines = dump([f"taps {t0} {t1} {_bits(r):016x} {PRECISION} {NWIN} {n}" for t0, t1, r, n in jobs])
    _check_taps(lines, jobs)


@needs_cxx
def test_tap_plan_where_the_time_is_within_a_few_ulp_of_an_integer(dump):
    """t * inc at or next to an integer: int() and the fraction behind it decide the centre sample and both table offsets."""
    jobs = []
    for r in RATIOS:
        inc = 1.0 / r
        t = np.arange(1, 400000, dtype=np.float64)
        time = t * inc
        near = np.abs(time - np.rint(time)) <= 4 * np.spacing(time)
        picks = t[near].astype(np.int64)
        assert picks.size >= 1, r
        picks = np.concatenate([picks[:300], picks[-300:]])
        jobs += [(int(p), int(p) + 1, r, 2 * 10 ** 6) for p in np.unique(picks)]
    inexact = [j for j in jobs if (j[0] * (1.0 / j[2])) != round(j[0] * (1.0 / j[2]))]
    assert inexact, "no output whose time is next to an integer without being one"
    lines = dump([f"taps {t0} {t1} {_bits(r):016x} {PRECISION} {NWIN} {n}" for t0, t1, r, n in jobs])
    _check_taps(lines, jobs)


# ---------------------------------------------------------------- the table and the restatement

def test_filter_table_is_its_formula(best):
    from xvector_amd import resample as rs
    assert rs.FILTERS == {"kaiser_best": ref.KAISER_BEST, "kaiser_fast": ref.KAISER_FAST}
    for name, kw in rs.FILTERS.items():
        win = rs.sinc_window(**kw)
        P, zeros, rolloff = 2 ** kw["precision"], kw["num_zeros"], kw["rolloff"]
        assert win.dtype == np.float64 and win.shape == (P * zeros + 1,) and np.array_equal(win, ref.sinc_window(**kw))
        assert win[0] == rolloff                                          # sinc(0) = 1 and the window's centre is 1
        # the sinc's zeros sit at multiples of P / rolloff entries: the sign changes follow them, one per zero, in order
        flips = np.nonzero(np.signbit(win[1:]) != np.signbit(win[:-1]))[0] + 1
        want = np.arange(1, int(zeros * rolloff) + 1) * P / rolloff
        assert flips.shape == want.shape and np.all(np.diff(flips) > 0), name
        assert np.all((flips >= want) & (flips < want + 1)), name         # the first entry past each zero
        last = rolloff * abs(np.sinc(rolloff * zeros)) / np.i0(kw["beta"])     # the window's end is 1 / I0(beta)
        assert abs(abs(win[-1]) - last) <= 1e-9 * last and abs(win[-1]) < 1e-4 * rolloff, name


@pytest.mark.parametrize("accumulate", ["float64", "float32"])
def test_vectorised_restatement_equals_the_double_loop(accumulate):
    fast = ref.sinc_window(**ref.KAISER_FAST)
    rng = np.random.default_rng(5)
    for ratio, n in [(2.0, 37), (1.0, 40), (16000 / 48000, 150), (44100 / 16000, 33), (1 / 1.1, 60), (16000 / 11025, 1), (1 / 3, 2)]:
        x = rng.standard_normal(n).astype(np.float32)
        a, b = ref.resample_loops(x, ratio, fast, 9, accumulate), ref.resample_row(x, ratio, fast, 9, accumulate)
        assert a.shape == b.shape == (int(n * ratio),) and np.array_equal(a, b), (ratio, n)
        if accumulate == "float32" and a.size:
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    out, lens = ref.resample(rng.standard_normal((3, 50)).astype(np.float32), [1 / 0.9, 1.0, 1 / 1.1], fast, 9, accumulate, lens=[50, 0, 31])
    assert list(lens) == [int(50 * (1 / 0.9)), 0, int(31 * (1 / 1.1))] and out.shape == (3, int(50 * (1 / 0.9)))
    assert not out[1].any() and not out[2, lens[2]:].any()


# (sr_orig, sr_new, the restatement's own error measured in fp64, the bar)
SINES = [(8000, 16000, 3.2e-8, 1e-6), (16000, 16000, 3.0e-8, 1e-6), (16000, 44100, 1.0e-7, 1e-6), (48000, 16000, 2.74e-3, 1e-2),
         (44100, 16000, 2.76e-3, 1e-2)]


@pytest.mark.parametrize("sr_orig,sr_new,measured,bar", SINES)
def test_restatement_resamples_a_sine_to_the_analytic_sine(best, sr_orig, sr_new, measured, bar):
    """A unit 1 kHz sine of 4000 samples against sin(2 pi 1000 t / sr_new), without the first and last 300 * max(1, ratio)
    outputs (the filter's edge).  Upsampling and equal rates: the restatement is 3e-8 .. 1e-7 off, the bar is 1e-6.
    Downsampling: the table step int(ratio * 512) is TRUNCATED (512 / 3 -> 170, as resampy 0.3.0 does), which stretches the
    filter by 170.67 / 170 and leaves 2.7e-3; the bar is 1e-2, about 3.5 times the restatement's own error."""
    ratio = float(sr_new) / sr_orig
    x = np.sin(2 * np.pi * 1000 * np.arange(4000) / sr_orig)
    y = ref.resample_row(x, ratio, best, 9, "float64")
    skip = int(300 * max(1.0, ratio))
    want = np.sin(2 * np.pi * 1000 * np.arange(y.shape[0]) / sr_new)
    err = np.abs(y - want)[skip:-skip].max()
    print(f"{sr_orig} -> {sr_new}: max |error| {err:.3e} (measured when written: {measured:.2e}; bar {bar:.0e})")
    assert y.shape[0] == int(4000 * ratio) and y.shape[0] > 3 * skip
    assert err <= bar


# ---------------------------------------------------------------- the C ABI without a device

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first


def _call(lib, ratios=(0.5,), **kw):
    import ctypes
    a = dict(x=P, x_dtype=0, ld_in=100, batch=2, n=100, lens=None, len_dtype=0, n_ratios=None, win=P, nwin=NWIN, precision=9,
             acc_mode=0, out=P + 0x10000, out_dtype=0, ld_out=50, out_cols=50, out_len=P, ws=P, ws_bytes=None, ratios_ptr=True)
    a.update(kw)
    if a["n_ratios"] is None:
        a["n_ratios"] = len(ratios)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = 1 << 20
    arr = (ctypes.c_double * max(1, len(ratios)))(*ratios)
    return lib.xvec_resample(a["x"], a["x_dtype"], a["ld_in"], a["batch"], a["n"], a["lens"], a["len_dtype"],
                             arr if a["ratios_ptr"] else None, a["n_ratios"], a["win"], a["nwin"], a["precision"], a["acc_mode"],
                             a["out"], a["out_dtype"], a["ld_out"], a["out_cols"], a["out_len"], a["ws"], a["ws_bytes"], None)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_resample_last_error().decode()
    need = lib.xvec_resample_workspace_bytes(2, 2)
    assert need >= 2 * 40 and need % 256 == 0 and lib.xvec_resample_workspace_bytes(2, 1) >= 40
    for batch, n_ratios in ((0, 1), (-1, 1), (4, 2), (4, 0), (1, 4)):
        assert lib.xvec_resample_workspace_bytes(batch, n_ratios) == 0, (batch, n_ratios)
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(batch=0), hip.ERR_ARG, "batch = 0: need at least one row"),
        (dict(n=0, ld_in=0), hip.ERR_ARG, "n = 0: need at least one sample"),
        (dict(out_cols=0, ld_out=0), hip.ERR_ARG, "out_cols = 0: need at least one output column"),
        (dict(n=2 ** 31, ld_in=2 ** 31), hip.ERR_TOO_LARGE, f"n = {2 ** 31} and out_cols = 50 must be at most 2^31 - 1"),
        (dict(x_dtype=2), hip.ERR_ARG, "x_dtype = 2: 0 (fp32) or 1 (int16)"),
        (dict(out_dtype=-1), hip.ERR_ARG, "out_dtype = -1: 0 (fp32) or 1 (fp64)"),
        (dict(acc_mode=2), hip.ERR_ARG, "acc_mode = 2: 0 (fp32 running sum) or 1 (fp64)"),
        (dict(len_dtype=3), hip.ERR_ARG, "len_dtype = 3: 0 (int64) or 1 (int32)"),
        (dict(ld_in=99), hip.ERR_ARG, "ld_in = 99 is smaller than n = 100"),
        (dict(ld_out=49), hip.ERR_ARG, "ld_out = 49 is smaller than out_cols = 50"),
        (dict(n_ratios=3), hip.ERR_ARG, "n_ratios = 3: one ratio for the batch or one per row (batch = 2)"),
        (dict(n_ratios=0), hip.ERR_ARG, "n_ratios = 0: one ratio for the batch or one per row (batch = 2)"),
        (dict(precision=-1), hip.ERR_ARG, "precision = -1 must be in 0 .. 20"),
        (dict(precision=21), hip.ERR_ARG, "precision = 21 must be in 0 .. 20"),
        (dict(nwin=512), hip.ERR_ARG, "nwin = 512: the table needs 2^precision + 1 = 513 .. 2^31 - 1 entries"),
        (dict(x=None), hip.ERR_ARG, "null pointer: x"),
        (dict(ratios_ptr=False), hip.ERR_ARG, "null pointer: ratios"),
        (dict(win=None), hip.ERR_ARG, "null pointer: win"),
        (dict(out=None), hip.ERR_ARG, "null pointer: out / out_len"),
        (dict(out_len=None), hip.ERR_ARG, "null pointer: out / out_len"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(ratios=(0.0,)), hip.ERR_ARG, "ratios[0] = 0 must be finite and positive"),
        (dict(ratios=(0.5, -1.0)), hip.ERR_ARG, "ratios[1] = -1 must be finite and positive"),
        (dict(ratios=(nan,)), hip.ERR_ARG, "ratios[0] = nan must be finite and positive"),
        (dict(ratios=(0.5, inf)), hip.ERR_ARG, "ratios[1] = inf must be finite and positive"),
        (dict(ratios=(0.001,)), hip.ERR_ARG, "ratios[0] = 0.001: step = int(ratio * 512) = 0, need at least 1"),
        (dict(ratios=(0.5, 0.52)), hip.ERR_ARG, "out_cols = 50 is smaller than int(n * ratios[1]) = 52"),
        (dict(ratios=(0.5, 0.5), ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
    ]
    for kwargs, code, text in cases:
        assert _call(lib, **kwargs) == code, kwargs
        assert err() == text, kwargs
    # the two host helpers
    for n, r in ((4000, 1 / 3), (4000, 16000 / 44100), (1, 0.5), (0, 2.0), (2 ** 31 - 1, 44100 / 16000)):
        assert lib.xvec_resample_out_len(n, r) == ref.num_out(n, r)
    for n, r in ((-1, 1.0), (5, 0.0), (5, -2.0), (5, nan), (5, inf)):
        assert lib.xvec_resample_out_len(n, r) == -1
    assert lib.xvec_resample_tile_span(1 / 3, NWIN, 9) == 255 * 3 + 1 + 2 * (NWIN // 170)
    for r, nwin, prec in ((0.001, NWIN, 9), (nan, NWIN, 9), (1.0, 512, 9), (1.0, NWIN, 21)):
        assert lib.xvec_resample_tile_span(r, nwin, prec) == -1


def test_resample_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    assert _call(lib, acc_mode=7) == hip.ERR_ARG
    assert lib.xvec_aug_normalize(None, 0, 0, 0, None) != hip.OK
    aug = lib.xvec_aug_last_error().decode()
    assert aug and lib.xvec_resample_last_error().decode() == "acc_mode = 7: 0 (fp32 running sum) or 1 (fp64)"
    assert _call(lib, ld_in=1) == hip.ERR_ARG
    assert lib.xvec_resample_last_error().decode() == "ld_in = 1 is smaller than n = 100"
    assert lib.xvec_aug_last_error().decode() == aug


def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    import xvector_amd as xa
    from xvector_amd import resample as rs
    consts = header_constants("xvec_resample.h", "XVEC_RESAMPLE_")
    assert consts == {"X_F32": rs.X_F32, "X_I16": rs.X_I16, "OUT_F32": rs.OUT_F32, "OUT_F64": rs.OUT_F64, "ACC_F32": rs.ACC_F32,
                      "ACC_F64": rs.ACC_F64, "LEN_I64": rs.LEN_I64, "LEN_I32": rs.LEN_I32, "TILE": rs.TILE, "SPAN_MAX": rs.SPAN_MAX,
                      "PRECISION_MAX": rs.PRECISION_MAX}
    assert xa.Resampler is rs.Resampler and xa.speed_perturb is rs.speed_perturb and xa.resample is rs
    r = rs.Resampler(48000, 16000)
    assert r.num_out(4000) == 1333 and r.ratio == 16000 / 48000 and rs.Resampler(16000, 44100).num_out(4000) == 11025
    assert rs.tile_span(1 / 3) == 255 * 3 + 1 + 2 * 192 <= rs.SPAN_MAX
    with pytest.raises(RuntimeError, match="HIP device only"):
        r(torch.zeros(2, 400))
    with pytest.raises(RuntimeError, match="HIP device only"):
        rs.speed_perturb(torch.zeros(2, 400), [0.9, 1.1])
    with pytest.raises(RuntimeError, match="HIP device only"):
        rs.resample(np.zeros(400, dtype=np.int16), 8000, 16000, device="cpu")
    with pytest.raises(ValueError, match="unknown filter"):
        rs.Resampler(8000, 16000, filter="sinc_best")
    with pytest.raises(ValueError, match="not a ratio"):
        rs.Resampler(16000 * 1024, 16000)                                 # step = int(512 / 1024) = 0


def test_drop_in_raises_the_package_s_error_on_an_empty_output():
    import xvector_amd as xa
    with pytest.raises(ValueError, match="Input signal length=2 is too small to resample from 48000->16000"):
        xa.resample(np.zeros(2, dtype=np.int16), 48000, 16000)
    with pytest.raises(ValueError, match="Input signal length=1 is too small"):
        xa.resample.resample(np.zeros((3, 1), dtype=np.float32), 16000, 8000)
    with pytest.raises(TypeError, match="int16 / float32"):
        xa.resample(np.zeros(100), 8000, 16000)
