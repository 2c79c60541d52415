"""CPU side of the MFCC probes (tests/mfcc_probe_ref.py): the helper's identities, its masks, and -- for every input the GPU
tests use -- that the fp32 reference ALONE (one real transform per frame, no pairing) stays inside the bar the GPU test applies to
the kernel, through the same check functions.  A correct fp32 kernel can therefore pass every case; and the tone probe does
notice a spectrum displaced by one bin or one filterbank weight off by 1 %."""
import numpy as np
import pytest

import mfcc_oracle as mo
import mfcc_probe_ref as pr

FLOAT_CASES = [(layout, db, kind) for layout in pr.LAYOUTS for db in pr.LEVELS_FLOAT for kind in pr.KINDS]
PCM_CASES = [(layout, scale) for layout in pr.LAYOUTS for scale in pr.PCM_SCALES]


@pytest.mark.parametrize("plan", list(pr.LOGMEL_PLANS))
def test_cepstra_invert_to_log_mel_energies(plan):
    kw = pr.LOGMEL_PLANS[plan]
    x = pr._speechlike(3000, 5)
    c = mo.mfcc(x, 16000, **kw)
    ref = pr.oracle_logmel_rows(x[None], **kw)[0]
    assert c.shape == ref.shape == (mo.num_frames(3000), kw["nfilt"])
    assert np.abs(pr.logmel_from_cepstra(c) - ref).max() <= 1e-9
    d = pr.dct_matrix(kw["nfilt"])
    assert np.allclose(d @ d.T, np.eye(kw["nfilt"]), atol=1e-13)
    assert np.allclose(mo.dct2_ortho(ref, 13), ref @ pr.dct_matrix(kw["nfilt"], 13).T, atol=1e-12)


def test_fp32_reference_is_the_oracle_in_float32():
    x = pr._speechlike(4000, 6)
    for kw in (pr.REFERENCE_CALL, dict(pr.REFERENCE_CALL, nfft=1024), *pr.LOGMEL_PLANS.values()):
        got, ref = pr.mfcc_fp32_unpaired(x, 16000, **kw), mo.mfcc(x, 16000, **kw)
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert pr.rowwise_rel(got, ref).max() <= 5e-6                       # float32 against float64: nothing else differs
    silent = pr.mfcc_fp32_unpaired(np.zeros(1000, np.float32), 16000, **pr.REFERENCE_CALL)
    assert np.allclose(silent, mo.mfcc(np.zeros(1000), 16000, **pr.REFERENCE_CALL), rtol=1e-6, atol=1e-4)   # (cepstra of a flat log-mel row: 0)


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_masks_name_the_quiet_and_the_loud_frames(layout):
    """Every sample an all-quiet frame reads -- the one before its first included, which the pre-emphasis reads -- is at the quiet
    level, every sample of an all-loud frame comes from the loud content, the remaining frames hold both; 16-bit PCM likewise."""
    for db, kind in ((60, "speech"), (120, "white"), (0, "pcm")):
        case = pr.level_case(layout, db, kind)
        B, n = case.x.shape
        assert case.quiet.shape == case.loud.shape == (B, mo.num_frames(n))
        assert case.quiet.sum() >= 4 and case.loud.sum() >= 4 and not (case.quiet & case.loud).any()
        level = 3 if kind == "pcm" else 1.0001 * pr.quiet_factor(db)
        is_quiet = np.abs(case.x.astype(np.float64)) <= level
        assert (case.x != 0).all() and (case.flat != 0).all()
        assert (np.abs(case.flat.astype(np.float64)) <= level).all()
        n_mixed = 0
        for b in range(B):
            for f in range(case.quiet.shape[1]):
                lo, hi = pr.frame_span(f, n)
                assert lo == max(160 * f - 1, 0) and hi == min(160 * f + 400, n) and hi > lo
                if case.quiet[b, f]:
                    assert is_quiet[b, lo:hi].all()
                    assert np.array_equal(case.x[b, lo:hi], case.flat[b, lo:hi])
                elif case.loud[b, f]:
                    assert not np.array_equal(case.x[b, lo:hi], case.flat[b, lo:hi])
                    assert np.abs(case.x[b, lo:hi].astype(np.float64)).max() > 30 * level
                else:
                    n_mixed += 1
                    assert is_quiet[b, lo:hi].any() and not is_quiet[b, lo:hi].all()
        assert (n_mixed > 0) == (layout == "step")


def test_step_rows_put_the_step_behind_an_even_and_an_odd_frame():
    case = pr.step_rows(80, "speech")
    last_quiet = [int(np.flatnonzero(case.quiet[r]).max()) for r in (0, 1)]
    first_quiet = [int(np.flatnonzero(case.quiet[r]).min()) for r in (2, 3)]
    assert last_quiet == [4, 5] and first_quiet == [7, 8]
    assert [int(np.flatnonzero(case.loud[r]).min()) for r in (0, 1)] == [7, 8]


@pytest.mark.parametrize("nfft", [512, 1024])
@pytest.mark.parametrize("layout,db,kind", FLOAT_CASES)
def test_fp32_reference_meets_the_level_bars(layout, db, kind, nfft):
    case = pr.level_case(layout, db, kind)
    kw = {**pr.REFERENCE_CALL, "nfft": nfft}
    pr.check_level_case(case, pr.fp32_rows(case.x, **kw), pr.fp32_rows(case.flat, **kw), pr.level_oracle(layout, db, kind, nfft),
                        f"fp32 reference, nfft {nfft}, {case.name}")


@pytest.mark.parametrize("nfft", [512, 1024])
@pytest.mark.parametrize("layout,scale", PCM_CASES)
def test_fp32_reference_meets_the_level_bars_on_pcm(layout, scale, nfft):
    case = pr.level_case(layout, 0, "pcm")
    kw = {**pr.REFERENCE_CALL, "nfft": nfft}
    pr.check_level_case(case, pr.fp32_rows(pr.as_float(case.x, scale), **kw), pr.fp32_rows(pr.as_float(case.flat, scale), **kw),
                        pr.level_oracle(layout, 0, "pcm", nfft, scale), f"fp32 reference, nfft {nfft}, scale {scale:.3g}, {case.name}")


def _probe_rows(which, nfft):
    return pr.tone_rows(nfft)[0] if which == "tones" else pr.edge_rows()[0]


@pytest.mark.parametrize("which", ["tones", "edges"])
@pytest.mark.parametrize("plan", list(pr.LOGMEL_PLANS))
def test_fp32_reference_meets_the_band_bars(plan, which):
    """By construction (the bar is 8 x its own error), and the bar separates: far below the 0.1 a displaced bin moves a band by."""
    kw = pr.LOGMEL_PLANS[plan]
    rows = _probe_rows(which, kw["nfft"])
    ref, bar, own = pr.logmel_bar(rows, kw)
    assert np.isfinite(ref).all() and 1e-5 <= bar <= 1e-2 and own <= bar / 8 + 1e-12
    pr.check_logmel(pr.fp32_rows(rows, **kw), ref, bar, f"fp32 reference, {plan}, {which}")


def test_tones_cover_every_bin_and_edges_sit_on_frame_ends():
    rows, bins = pr.tone_rows(512)
    assert rows.shape == (513, 400) and rows.dtype == np.float32
    assert np.array_equal(bins[:257], np.arange(257)) and np.allclose(bins[257:], np.arange(256) + 0.37)
    spec = np.abs(np.fft.rfft(rows[:257].astype(np.float64), 512, axis=1))
    assert np.array_equal(spec.argmax(axis=1), np.arange(257))              # tone k peaks in bin k
    x, at = pr.edge_rows()
    assert at == [1039, 1040, 1199, 1200] and all(x[r, s] > 0.99 for r, s in enumerate(at))
    e = np.stack([mo.fbank(w.astype(np.float64), 16000, nfilt=26, nfft=512)[1] for w in x])
    assert e[0, 4] > 300 * e[1, 4] and e[2, 5] > 300 * e[3, 5]              # frame f with and without the impulse


@pytest.mark.parametrize("plan", list(pr.LOGMEL_PLANS))
def test_tone_probe_notices_a_displaced_bin_and_a_wrong_weight(plan):
    """The defects the probe exists for, put into the fp32 reference and through the same assertion: the spectrum rolled by
    one bin, and ONE filterbank weight changed by 1 %."""
    kw = pr.LOGMEL_PLANS[plan]
    rows = pr.tone_rows(kw["nfft"])[0]
    ref, bar, _ = pr.logmel_bar(rows, kw)
    for roll in (1, -1):
        with pytest.raises(AssertionError, match="log-mel off by"):
            pr.check_logmel(pr.fp32_rows(rows, roll_bins=roll, **kw), ref, bar, f"{plan}, spectrum rolled by {roll}")
    fb = mo.get_filterbanks(kw["nfilt"], kw["nfft"], 16000, kw.get("lowfreq", 0), kw.get("highfreq", None))
    for band in (0, kw["nfilt"] // 2, kw["nfilt"] - 1):
        for k in (int(np.argmax(fb[band])), int(np.flatnonzero(fb[band])[0]), int(np.flatnonzero(fb[band])[-1])):    # peak and both edges
            bad = fb.copy()
            bad[band, k] *= 1.01
            with pytest.raises(AssertionError, match="log-mel off by"):
                pr.check_logmel(pr.fp32_rows(rows, fb=bad, **kw), ref, bar, f"{plan}, weight ({band}, {k}) off by 1 %")
