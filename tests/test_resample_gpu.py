"""The resampling kernel (csrc/resample.hip) against the numpy restatement of resampy's arithmetic (tests/resample_ref.py) on the
GPU.  Every comparison is EXACT: torch.equal on the fp64 output, and on the fp32 output against the reference rounded once -- a
tolerance would hide a fused multiply-add or a reordered sum.  Rows are a few hundred to a few thousand samples: the edges are
those of the tile (XVEC_RESAMPLE_TILE outputs per block), of the staged input span (XVEC_RESAMPLE_SPAN_MAX samples of LDS), of a
wing that does not fit the row, and of rows without outputs."""
import functools

import numpy as np
import pytest
import torch

import resample_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = [2.0, 1.0, 16000 / 48000, 16000 / 44100, 44100 / 16000, 16000 / 22050, 16000 / 11025, 1 / 0.9, 1 / 1.1]
NP_OUT = {torch.float32: np.float32, torch.float64: np.float64}


@functools.lru_cache(maxsize=None)
def _best():
    return ref.sinc_window(**ref.KAISER_BEST)


def _pcm(shape, seed):
    """int16 samples with a full-scale range (what wavfile.read yields)."""
    return np.random.default_rng(seed).integers(-32768, 32768, size=shape, dtype=np.int64).astype(np.int16)


def _run(x, ratios, lens=None, accumulate="float64", out_dtype=torch.float64, **kw):
    from xvector_amd import resample as rs
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out, out_lens = rs.resample_rows(x, ratios, lens, "kaiser_best", accumulate, out_dtype, **kw)
    torch.cuda.synchronize()
    return out, out_lens


def _same(out, out_lens, want, want_lens, what=""):
    """Exact: the reference (float64) rounded once to the output's dtype; NaN matches NaN."""
    got = out.cpu().numpy()
    want = want.astype(NP_OUT[out.dtype])
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(out_lens.cpu().numpy().astype(np.int64), want_lens), (what, out_lens, want_lens)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    a, b = np.where(nan, 0, got), np.where(nan, 0, want)
    bad = np.nonzero(a != b)
    assert bad[0].size == 0, (what, f"{bad[0].size} outputs differ; first at {bad[0][0], bad[1][0]}: {a[bad][0]!r} != {b[bad][0]!r}")
    assert np.array_equal(np.signbit(a), np.signbit(b)), what


@pytest.mark.parametrize("ratio", RATIOS)
def test_every_mode_and_dtype_equals_the_restatement_bit_for_bit(ratio):
    pcm = _pcm((2, 700), 11)
    for accumulate in ("float64", "float32"):
        want, want_lens = ref.resample(pcm, ratio, _best(), 9, accumulate)
        assert want_lens[0] == int(700 * ratio) == want.shape[1]
        outs = {}
        for x in (pcm, pcm.astype(np.float32)):
            for out_dtype in (torch.float64, torch.float32):
                out, out_lens = _run(x, [ratio], None, accumulate, out_dtype)
                _same(out, out_lens, want, want_lens, (ratio, accumulate, x.dtype, out_dtype))
                outs[(x.dtype.name, out_dtype)] = out
        for out_dtype in (torch.float64, torch.float32):                     # int16 input == the same values as fp32
            assert torch.equal(outs[("int16", out_dtype)], outs[("float32", out_dtype)])
        if accumulate == "float32":                                          # every partial sum was a float32: so is the result
            assert torch.equal(outs[("int16", torch.float64)], outs[("int16", torch.float32)].double())


def _rows_with_n_out(ratio, targets):
    sizes = []
    for target in targets:
        n = next(n for n in range(1, 10 * target + 10) if ref.num_out(n, ratio) == target)
        sizes.append(n)
    return sizes


@pytest.mark.parametrize("ratio", [1.0, 16000 / 48000, 16000 / 22050, 2.0])
def test_output_counts_at_the_tile_edges(ratio):
    """n_out = tile - 1, tile, tile + 1 and two tiles + 1 (at ratio 2, where n_out is even: tile - 2, tile, tile + 2, two
    tiles, two tiles + 2)."""
    from xvector_amd import resample as rs
    T = rs.TILE
    sizes = [T // 2 - 1, T // 2, T // 2 + 1, T, T + 1] if ratio == 2.0 else _rows_with_n_out(ratio, [T - 1, T, T + 1, 2 * T + 1])
    for n in sizes:
        x = np.random.default_rng(n).standard_normal((2, n)).astype(np.float32)
        for accumulate in ("float64", "float32"):
            want, want_lens = ref.resample(x, ratio, _best(), 9, accumulate)
            out, out_lens = _run(x, [ratio], None, accumulate, torch.float64)
            _same(out, out_lens, want, want_lens, (ratio, n, accumulate))


def test_rows_at_the_staged_span_limit_and_just_below_it():
    """The smallest ratio whose tiles are still staged in LDS and the next one down, which reads the row from memory, as two rows
    of one launch and each on its own: the same bits as the restatement either way."""
    from xvector_amd import resample as rs
    lo, hi = 0.03, 0.06                                                      # tile_span(lo) > SPAN_MAX >= tile_span(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if rs.tile_span(mid) <= rs.SPAN_MAX else (mid, hi)
    assert rs.tile_span(lo) > rs.SPAN_MAX >= rs.tile_span(hi) > rs.SPAN_MAX - 64 and hi - lo < 1e-9
    n = 3 * rs.SPAN_MAX
    x = _pcm((2, n), 3)
    assert ref.num_out(n, lo) > 4 * rs.TILE                                  # tiles in the row's middle with both wings whole
    for accumulate in ("float64", "float32"):
        want, want_lens = ref.resample(x, [hi, lo], _best(), 9, accumulate)
        out, out_lens = _run(x, [hi, lo], None, accumulate, torch.float64)
        _same(out, out_lens, want, want_lens, accumulate)
        for b, r in enumerate((hi, lo)):
            one, one_lens = _run(x[b:b + 1], [r], None, accumulate, torch.float64)
            assert torch.equal(one[0, :want_lens[b]], out[b, :want_lens[b]]) and int(one_lens[0]) == want_lens[b]


@pytest.mark.parametrize("ratio,sizes", [(2.0, (1, 2, 63, 64, 65)), (1.0, (1, 2, 63, 64, 65)), (44100 / 16000, (1, 2, 63, 64, 65)),
                                         (1 / 3, (1, 2, 63, 64, 65, 191, 192, 193))])
def test_rows_shorter_than_a_wing(ratio, sizes):
    """Both min(...) clips of the tap counts are active on every output (a wing is 64 taps, 192 at ratio 1 / 3)."""
    for n in sizes:
        x = _pcm((3, n), 100 + n)
        for accumulate in ("float64", "float32"):
            want, want_lens = ref.resample(x, ratio, _best(), 9, accumulate)
            for out_dtype in (torch.float64, torch.float32):
                out, out_lens = _run(x, [ratio], None, accumulate, out_dtype)
                _same(out, out_lens, want, want_lens, (ratio, n, accumulate, out_dtype))


@pytest.mark.parametrize("len_dtype", [torch.int64, torch.int32])
def test_ragged_batch_in_one_launch(len_dtype):
    ratio, n = 1 / 3, 700
    lens = [0, 1, 2, 700, 3, 350]
    assert [ref.num_out(v, ratio) for v in lens] == [0, 0, 0, 233, 1, 116]
    x = np.random.default_rng(9).standard_normal((len(lens), n)).astype(np.float32)
    want, want_lens = ref.resample(x, ratio, _best(), 9, "float64", lens=lens)
    for b, v in enumerate(lens):
        x[b, v:] = np.nan                                                    # padding: never read
    cols = ref.num_out(n, ratio)
    out = torch.full((len(lens), cols), float("nan"), dtype=torch.float64, device=DEV)
    got, got_lens = _run(x, [ratio], torch.tensor(lens, dtype=len_dtype, device=DEV), "float64", torch.float64, out=out)
    assert got.data_ptr() == out.data_ptr() and got_lens.dtype == len_dtype
    assert not torch.isnan(out).any()
    for b, v in enumerate(want_lens):
        assert not out[b, v:].any()                                          # exactly 0 past out_len[b]
    _same(out, got_lens, want, want_lens)


def test_speed_perturb_equals_single_ratio_calls():
    from xvector_amd import resample as rs
    factors = [0.9, 1.0, 1.1]
    pcm = _pcm((3, 900), 21)
    x = torch.from_numpy(pcm).to(DEV)
    lens = [900, 640, 777]
    for kw in (dict(), dict(accumulate="float64", out_dtype=torch.float64)):
        acc = kw.get("accumulate", "float32")
        out, out_lens = rs.speed_perturb(x, factors, **kw)
        want, want_lens = ref.resample(pcm, [1 / f for f in factors], _best(), 9, acc)
        assert out.shape == (3, 1000) and list(want_lens) == [1000, 900, 818]
        _same(out, out_lens, want, want_lens, kw)
        for b, f in enumerate(factors):
            one, _ = rs.resample_rows(x[b:b + 1], [1 / f], None, "kaiser_best", acc, out.dtype)
            assert torch.equal(one[0], out[b, :one.shape[1]]) and not out[b, one.shape[1]:].any()
        rag, rag_lens = rs.speed_perturb(x, factors, lens=lens, **kw)
        want, want_lens = ref.resample(pcm, [1 / f for f in factors], _best(), 9, acc, lens=lens)
        _same(rag, rag_lens, want, want_lens, (kw, "ragged"))


@pytest.mark.parametrize("in_dtype,out_dtype", [(np.float32, torch.float32), (np.int16, torch.float64), (np.float32, torch.float64)])
def test_strided_rows_and_a_misaligned_base(in_dtype, out_dtype):
    ratio, B, n, ld = 44100 / 16000, 3, 301, 333
    cols, ld_out = ref.num_out(n, ratio), ref.num_out(n, ratio) + 7
    x = _pcm((B, n), 5).astype(in_dtype)
    buf = torch.full((B * ld + 1,), 77, dtype=torch.from_numpy(x).dtype, device=DEV)
    xin = buf[1:].view(B, ld)[:, :n]                                         # base one element off the allocation's alignment
    xin.copy_(torch.from_numpy(x))
    obuf = torch.full((B * ld_out + 1,), -5.0, dtype=out_dtype, device=DEV)
    oview = obuf[1:].view(B, ld_out)
    out, out_lens = _run(xin, [ratio], None, "float32", out_dtype, out=oview[:, :cols])
    assert xin.stride(0) == ld and out.stride(0) == ld_out and out.data_ptr() == oview.data_ptr()
    want, want_lens = ref.resample(x, ratio, _best(), 9, "float32")
    _same(out, out_lens, want, want_lens)
    assert (oview[:, cols:] == -5.0).all() and obuf[0] == -5.0               # the sentinel columns are untouched
    assert (buf[1:].view(B, ld)[:, n:] == 77).all()


def test_two_runs_are_bit_identical_and_the_workspace_s_contents_never_matter():
    from xvector_amd import hip
    x = _pcm((3, 800), 8)
    ratios = [1 / 0.9, 1 / 3, 2.0]
    need = int(hip.lib.xvec_resample_workspace_bytes(3, 3))
    assert need > 0
    first, first_lens = _run(x, ratios, None, "float32", torch.float32)
    again, again_lens = _run(x, ratios, None, "float32", torch.float32)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)            # exactly the reported size, poisoned
    third, third_lens = _run(x, ratios, None, "float32", torch.float32, workspace=ws)
    assert torch.equal(first, again) and torch.equal(first, third)
    assert torch.equal(first_lens, again_lens) and torch.equal(first_lens, third_lens)
    want, want_lens = ref.resample(x, ratios, _best(), 9, "float32")
    _same(first, first_lens, want, want_lens)


@pytest.mark.parametrize("ratio", [2.0, 1 / 3])
def test_nan_and_inf_reach_only_the_outputs_whose_taps_touch_them(ratio):
    n, nwin = 1500, _best().shape[0]
    x = np.random.default_rng(2).standard_normal((3, n)).astype(np.float32)
    x[0, 700] = np.nan
    x[1, 40] = np.inf
    x[2, 1499] = -np.inf
    want, want_lens = ref.resample(x, ratio, _best(), 9, "float64")
    out, out_lens = _run(x, [ratio], None, "float64", torch.float64)
    _same(out, out_lens, want, want_lens)
    got = out.cpu().numpy()
    for b, pos in enumerate((700, 40, 1499)):
        touched = np.zeros(want.shape[1], dtype=bool)
        for t in range(want.shape[1]):
            n0, _, _, i_max, _, _, k_max = ref.tap_plan(t, ratio, 9, nwin, n)
            touched[t] = n0 - i_max < pos <= n0 + max(k_max, 0)
        assert 0 < touched.sum() < touched.size
        assert np.isfinite(got[b, ~touched]).all() and not np.isfinite(got[b, touched]).any()
    assert np.isnan(got[0]).sum() == np.isnan(want[0]).sum() > 0


def test_telephone_pcm_through_the_resampler_into_the_mfcc_front_end():
    """8 kHz PCM -> Resampler -> MfccFrontEnd: num_frames(num_out(n)) frames, and the features of the reference-resampled wave
    inside the MFCC tests' own bar (tests/test_mfcc.py: 1e-4 per frame norm-wise, 1e-3 element-wise)."""
    import mfcc_oracle as mo
    import xvector_amd as xa
    from conftest import assert_parity
    n = 4000
    t = np.arange(n) / 8000.0
    rng = np.random.default_rng(4)
    waves = np.stack([np.sin(2 * np.pi * (200 + 90 * b) * t) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(n)
                      for b in range(2)])
    pcm = np.round(waves / np.abs(waves).max() * 20000).astype(np.int16)
    rs, fe = xa.Resampler(8000, 16000, device=DEV), xa.MfccFrontEnd()
    up = rs(torch.from_numpy(pcm).to(DEV))
    feats = fe(up)
    want, _ = ref.resample(pcm, 2.0, _best(), 9, "float32")
    assert up.dtype == torch.float32 and up.shape == (2, rs.num_out(n)) == (2, 8000)
    assert np.array_equal(up.cpu().numpy(), want.astype(np.float32))
    assert feats.shape == (2, fe.num_frames(rs.num_out(n)), 24) and fe.num_frames(8000) == mo.num_frames(8000)
    ref_feats = np.stack([mo.mfcc(w, 16000, numcep=24, nfilt=26, nfft=512) for w in want.astype(np.float32)])
    assert_parity(feats.cpu().numpy(), ref_feats, 1e-4, "mfcc of the resampled PCM", elem_tol=1e-3)
    # and the numpy drop-in for the reference's call
    y = xa.resample(pcm[0], 8000, 16000)
    assert y.dtype == np.float32 and np.array_equal(y, want[0].astype(np.float32))
