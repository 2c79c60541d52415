"""Waveform augmentation on the device (include/xvec_augment.h, xvector_amd.augment) against tests/augment_ref.py and the
reference's own run (tests/golden/g9_augment.npz); everything goes through the package and so through the C ABI.

Bars, none of them tuned:
  mix gains     1e-14 relative: a handful of correctly rounded fp64 operations on exact integer sums
  mix samples   2^-23 |ref|: one fp32 rounding of an fp64 value (2^-24), doubled
  reverb        augment_ref.reverb_bound: (K + 8) 2^-24 (|x| * |h|) per output of the K-tap convolution (an fp32 sum of K
                exact products, in any order), carried through the scale max|x| / max|c| and the add, plus 2^-22 |ref| for the
                epilogue's roundings.  The largest ratio to that bound seen is recorded in profiles/augment_timing.txt.
  normalize     2^-22 absolute: outputs lie in [0, 1], three fp32 roundings
  fixture       the stages chained as the reference chains them; each output passes through normalize, so the bar is the
                stage's own bar carried through (y - min) / range (four times the error over the range) plus 2^-22."""
import numpy as np
import pytest
import torch

import augment_ref as ar
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def g9():
    return load_golden("g9_augment.npz")


@pytest.fixture(scope="module")
def aug9(g9):
    from xvector_amd.augment import WaveAugmenter
    return WaveAugmenter(g9["pool"], g9["pool_len"], g9["rirs"], g9["rir_len"], device=DEV)


def _plan(ops, srcs, rir_index):
    from xvector_amd.augment import OP_DTYPE, SRC_DTYPE, AugmentPlan
    return AugmentPlan(np.array([(u, off, ln, f, k, 0, r) for u, off, ln, f, k, r in ops], dtype=OP_DTYPE),
                       np.array(srcs, dtype=SRC_DTYPE), rir_index)


def _padded(x, pad=37):
    """x [B, n] as a view into a sentinel-filled buffer with row stride n + 2 pad, and the buffer."""
    B, n = x.shape
    buf = torch.full((B + 2, n + 2 * pad), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[1:B + 1, pad:pad + n]
    view.copy_(torch.as_tensor(x, dtype=torch.float32))
    return view, buf


def _padding_untouched(buf, B, n, pad=37):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:B + 1, pad:pad + n] = False
    return bool((buf[mask] == SENTINEL).all())


def _waves(B, n, seed, scale=6000.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, n)) * scale).astype(np.int16).astype(np.float32) + \
        rng.choice([0.0, 0.25, -0.5], size=(B, n)).astype(np.float32)          # not all integer-valued: trunc matters


# ---------------------------------------------------------------- the reference's own outputs

def test_fixture_kinds_against_the_reference(g9, aug9):
    from test_augment import _plan_of_case
    for case in range(len(g9["inputs"])):
        kind, plan = _plan_of_case(g9, case)
        x = g9["inputs"][case][None]
        got = aug9(torch.from_numpy(x).to(DEV), plan).cpu().numpy().astype(np.float64)[0]
        want = g9["outputs"][case]
        y, _ = ar.mix(x, g9["pool"], g9["pool_len"], plan.ops, plan.srcs)
        if kind == "rir":
            r = int(plan.rir_index[0])
            bound, y0 = ar.reverb_bound(y[0], g9["rirs"][r][:g9["rir_len"][r]])
            stage = bound.max()
        else:
            y0 = y[0]
            stage = 2.0 ** -23 * np.abs(y0).max()
        bar = 4 * stage / (y0.max() - y0.min()) + 2.0 ** -22 + (1e-7 if kind == "rir" else 0.0)   # 1e-7: the reference's fp32 FFT
        err = np.abs(got - want).max()
        print(f"case {case} {kind}: |got - reference| = {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (case, kind, err, bar)


# ---------------------------------------------------------------- mix

def _mix_case(B, n, seed, ops, srcs, pool, pool_len):
    from xvector_amd.augment import WaveAugmenter
    x = _waves(B, n, seed)
    plan = _plan(ops, srcs, [-1] * B)
    aug = WaveAugmenter(pool, pool_len, device=DEV)
    got = aug.mix(torch.from_numpy(x).to(DEV), plan)
    ref, gains = ar.mix(x, pool, pool_len, plan.ops, plan.srcs)
    g = aug.last_gains.cpu().numpy()
    assert aug.status()[0] == 0
    rel = np.abs(g - gains) / np.abs(gains)
    print(f"B={B} n={n}: gains rel err {rel.max():.3e}")
    assert (rel <= 1e-14).all(), (g, gains)
    gotn = got.cpu().numpy().astype(np.float64)
    assert (np.abs(gotn - ref) <= 2.0 ** -23 * np.abs(ref)).all(), np.abs(gotn - ref).max()
    return x, gotn, aug, plan


def _pool(R, m, seed, lens=None):
    rng = np.random.default_rng(seed)
    pool = (rng.standard_normal((R, m)) * 3000).astype(np.int16)
    lens = np.full(R, m) if lens is None else np.asarray(lens)
    for r in range(R):
        pool[r, lens[r]:] = 0
    return pool, lens


@pytest.mark.parametrize("B,n", [(1, 2400), (3, 2401)])
def test_mix_shapes(B, n):
    pool, lens = _pool(9, 3000, 1, [3000, 2000, 2500, 3000, 100, 3000, 2999, 1500, 3000])
    pool[8] = 0                                                              # an all-zero clip
    ops = [(0, 0, n, 0, 1, 10 ** 0.5)]
    srcs = [(0, 17)]
    if B == 3:
        # utt 0: one clip; utt 1: no ops; utt 2: the three overlapping noise ops, an op of length 1, seven summed speakers,
        # an all-zero clip
        srcs += [(1, 0), (2, 100), (3, 5)]                                   # 1..3: noise
        ops += [(2, 0, 800, 1, 1, 10 ** 0.3), (2, 1, 800, 2, 1, 1.0), (2, 2, 800, 3, 1, 10 ** 1.5)]
        srcs += [(4, 3)]
        ops += [(2, n - 1, 1, 4, 1, 10 ** 0.7)]                              # length 1, the last sample
        srcs += [(r, 10 * r) for r in range(7)]                              # 5..11: seven speakers, some end early
        ops += [(2, 0, n, 5, 7, 10 ** 1.3)]
        srcs += [(8, 0)]
        ops += [(2, 100, 500, 12, 1, 10 ** 0.5)]                             # all-zero noise: gain finite, output trunc(x)
    x, got, aug, plan = _mix_case(B, n, 5, ops, srcs, pool, lens)
    if B == 3:
        assert np.array_equal(got[1], x[1])                                  # no ops: untouched
        assert np.isfinite(aug.last_gains.cpu().numpy()).all()
        before = ar.mix(x, pool, lens, plan.ops[:-1], plan.srcs)[0][2, 100:600]
        assert np.array_equal(got[2, 100:600], np.trunc(before).astype(np.float32))
        # the same pool as fp32: bit-identical
        from xvector_amd.augment import WaveAugmenter
        got32 = WaveAugmenter(pool.astype(np.float32), lens, device=DEV).mix(torch.from_numpy(x).to(DEV), plan)
        assert np.array_equal(got32.cpu().numpy(), got.astype(np.float32))


def test_mix_full_length_row_and_repeatability():
    n = 48000
    pool, lens = _pool(4, 60000, 2, [60000, 30000, 48000, 50000])
    ops = [(0, 0, n, 0, 3, 10 ** 1.1), (0, 0, 16000, 3, 1, 10 ** 0.2), (0, 1, 16000, 3, 1, 10 ** 0.2)]
    srcs = [(0, 1234), (1, 0), (2, 0), (3, 999)]
    x, got, aug, plan = _mix_case(1, n, 6, ops, srcs, pool, lens)
    view, buf = _padded(x)
    aug._ws.fill_(0xFF)                                                      # NaN bytes in the workspace
    aug.mix(view, plan, inplace=True)
    assert np.array_equal(view.cpu().numpy().astype(np.float64), got) and _padding_untouched(buf, 1, n)


def test_mix_skips_and_counts_bad_sources():
    """Rows outside the pool and a negative start contribute zeros and are counted; nothing outside the pool is read."""
    from xvector_amd.augment import WaveAugmenter
    pool, lens = _pool(3, 1000, 3)
    x = _waves(2, 900, 7)
    srcs = [(0, 0), (3, 0), (-1, 0), (1, -5), (2, 50)]
    plan = _plan([(0, 0, 900, 0, 5, 10.0), (1, 0, 900, 1, 1, 10.0)], srcs, [-1, -1])
    aug = WaveAugmenter(pool, lens, device=DEV)
    got = aug.mix(torch.from_numpy(x).to(DEV), plan).cpu().numpy().astype(np.float64)
    assert aug.status()[0] == 4                                              # three in op 0, one in op 1
    ref, _ = ar.mix(x, pool, lens, plan.ops, plan.srcs)                      # the restatement skips them too
    assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref)).all()
    assert np.array_equal(got[1], np.trunc(x[1]))                            # only a skipped source: zero noise


# ---------------------------------------------------------------- reverb

def _reverb_check(x, rirs, rir_len, idx, record=None):
    from xvector_amd.augment import WaveAugmenter
    aug = WaveAugmenter(rirs=rirs, rir_len=rir_len, device=DEV)
    view, buf = _padded(x)
    got = aug.reverb(view, idx, inplace=True)
    gotn = got.cpu().numpy().astype(np.float64)
    assert _padding_untouched(buf, *x.shape) and aug.status()[1] == 0
    worst = 0.0
    for b, r in enumerate(idx):
        if r < 0:
            assert np.array_equal(gotn[b], x[b].astype(np.float64))
            continue
        bound, ref = ar.reverb_bound(x[b], rirs[r][:rir_len[r]])
        ratio = (np.abs(gotn[b] - ref) / np.maximum(bound, 1e-300)).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b, r, ratio)
    print(f"reverb n={x.shape[1]} L={list(rir_len)}: largest error / bound = {worst:.3f}")
    again = aug.reverb(torch.from_numpy(x).to(DEV), idx)                       # repeat, contiguous rows, fresh copy
    assert np.array_equal(again.cpu().numpy(), got.cpu().numpy())
    return gotn, worst


def _rirs(lens, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(lens), max(lens)), dtype=np.float32)
    for r, L in enumerate(lens):
        out[r, :L] = (rng.standard_normal(L) * np.exp(-np.arange(L) / max(L / 6.0, 1.0))).astype(np.float32)
    return out


@pytest.mark.parametrize("n,lens", [(2400, [31, 32, 33]), (2400, [1001, 3001, 7]), (2413, [33, 1001, 100])])
def test_reverb_shapes(n, lens):
    """Tap counts around the 32-tap block, more taps than samples, n not a multiple of 32; the middle row has no rir."""
    x = _waves(3, n, 11)
    rirs = _rirs(lens, 12)
    _reverb_check(x, rirs, lens, [0, -1, 1])
    _reverb_check(x[:1], rirs, lens, [2])


def test_reverb_unit_impulse_doubles_exactly():
    x = _waves(2, 2400, 13)
    got, _ = _reverb_check(x, np.ones((1, 1), dtype=np.float32), [1], [0, 0])
    assert np.array_equal(got, 2.0 * x.astype(np.float64))


def test_reverb_full_size_row():
    x = _waves(1, 48000, 14)
    _reverb_check(x, _rirs([4000], 15), [4000], [0])


def test_reverb_peak_in_the_tail():
    """max|c| lies past the first n outputs: a kernel that only forms c[:n] scales wrongly."""
    n, L = 2400, 1001
    x = np.zeros((1, n), dtype=np.float32)
    x[0, -100:] = _waves(1, 100, 16)[0]
    h = np.zeros((1, L), dtype=np.float32)
    h[0, 0], h[0, L - 1] = 0.1, 1.0
    c = ar.conv_full(x[0], h[0])
    assert np.abs(c).argmax() >= n
    _reverb_check(x, h, [L], [0])


def test_reverb_counts_out_of_range_rirs_and_degenerate_rows():
    from xvector_amd.augment import WaveAugmenter
    x = _waves(4, 1000, 17)
    x[2] = 0.0                                                               # an all-zero utterance: NaN, as the reference
    rirs = _rirs([50, 60], 18)
    rirs = np.concatenate([rirs, np.zeros((1, 60), dtype=np.float32)])       # an all-zero response
    aug = WaveAugmenter(rirs=rirs, rir_len=[50, 60, 60], device=DEV)
    got = aug.reverb(torch.from_numpy(x).to(DEV), [3, 2, 0, 1]).cpu().numpy()
    assert aug.status()[1] == 1 and np.array_equal(got[0], x[0])             # index 3 of 3: left alone and counted
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    bound, ref = ar.reverb_bound(x[3], rirs[1])
    assert (np.abs(got[3] - ref) <= bound).all()


# ---------------------------------------------------------------- normalize, composition

def test_normalize():
    from xvector_amd.augment import WaveAugmenter
    aug = WaveAugmenter(device=DEV)
    for B, n in ((1, 2400), (3, 2401), (2, 48000)):
        x = _waves(B, n, 20 + B)
        if B == 3:
            x[1] = 42.0                                                      # a constant row: NaN in that row only
        view, buf = _padded(x)
        got = aug.normalize(view, inplace=True).cpu().numpy()
        assert _padding_untouched(buf, B, n)
        for b in range(B):
            if B == 3 and b == 1:
                assert np.isnan(got[b]).all()
                continue
            ref = ar.normalize(x[b])
            assert np.abs(got[b] - ref).max() <= 2.0 ** -22
            assert got[b][x[b].argmin()] == 0.0 and got[b][x[b].argmax()] == 1.0
        assert np.array_equal(aug.normalize(torch.from_numpy(x).to(DEV)).cpu().numpy(), got, equal_nan=True)


def test_composition_feeds_the_front_end(g9):
    import mfcc_oracle as mo
    import xvector_amd as xa
    from conftest import assert_parity
    import random
    n, B = 48000, 4
    pool, lens = _pool(6, 50000, 30, [50000, 20000, 48000, 50000, 16000, 30000])
    rirs = _rirs([4000, 800], 31)
    aug = xa.WaveAugmenter(pool, lens, rirs, [4000, 800], device=DEV)
    plan = xa.AugmentPlan.draw(["music", "rir", "noise", "speech"], n, [0, 1], [2, 3], [4, 5], 2, rng=random.Random(1),
                               pool_len=lens)
    fe = xa.MfccFrontEnd()
    x = _waves(B, n, 32)
    feats = fe(aug(torch.from_numpy(x).to(DEV), plan))
    assert feats.shape == (B, 299, 24) and bool(torch.isfinite(feats).all())
    assert aug.status() == (0, 0)
    got = fe(aug.normalize(torch.from_numpy(x).to(DEV))).cpu().numpy()
    ref = np.stack([mo.mfcc(ar.normalize(w), 16000, numcep=24, nfilt=26, nfft=512) for w in x])
    assert_parity(got, ref, 1e-4, "mfcc of normalised waves", elem_tol=1e-3)      # the MFCC tests' own bar (test_mfcc.py)
