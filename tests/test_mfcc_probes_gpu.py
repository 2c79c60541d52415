"""The MFCC kernels (csrc/mfcc.hip) on the probes of tests/mfcc_probe_ref.py, in the three forms a plan can take: the nfft-512
kernel with the banded (2) and the dense (1) filterbank and the general kernel (0).

Level steps inside a pair: both kernels transform two frames as one complex signal, and a quiet frame used to receive its loud
partner's rounding noise (1.2e-3 row-wise at 80 dB, 0.13 at 120 dB); pair_scale in mfcc.hip brings the quiet frame to its
partner's level first.  The quiet frames are held to the path's bar ALONE, taken out of the output with their mask.

Band by band: with numcep = nfilt and no lifter the output inverts to the log-mel spectrum, and a pure tone says where its energy
went -- a bin in the wrong place (the three radix-8 digit steps, the split's partner-lane map, lane 0's pairing), a wrong weight
at a triangle's edge, a wrong bin 0 or nfft/2 move a band by 0.1 and more; the bar is 8 x the fp32 reference's own error.

tests/test_mfcc_probes.py shows on the CPU that the fp32 reference alone meets each of these bars on each of these inputs
(none had to be dropped or changed for it).  Measured figures, parent build and this one: profiles/mfcc_probe_errors.txt."""
import os

import numpy as np
import pytest
import torch

import mfcc_probe_ref as pr

pytestmark = pytest.mark.gpu

FORMS = {"banded": (2, dict()), "dense": (1, dict()), "general": (0, dict(nfft=1024))}
# band-by-band plans by kernel form: the reference's nfft = 512 and a telephone band on both filterbank forms, nfft = 1024 general
LOGMEL_FORMS = [("ref512", "banded"), ("ref512", "dense"), ("tel512", "banded"), ("tel512", "dense"), ("gen1024", "general")]


def _front_end(form, **kw):
    """A plan in the asked form (XVEC_MFCC_FILTERBANK is read at create time), kernel_form() asserted."""
    import xvector_amd as xa
    want = FORMS[form][0]
    old = os.environ.pop("XVEC_MFCC_FILTERBANK", None)
    try:
        if form == "dense":
            os.environ["XVEC_MFCC_FILTERBANK"] = "dense"
        fe = xa.MfccFrontEnd(**kw)
    finally:
        os.environ.pop("XVEC_MFCC_FILTERBANK", None)
        if old is not None:
            os.environ["XVEC_MFCC_FILTERBANK"] = old
    assert fe.kernel_form() == want, (form, kw, fe.kernel_form())
    return fe


@pytest.fixture(scope="module")
def level_front_ends():
    return {form: _front_end(form, **kw) for form, (_, kw) in FORMS.items()}


def _run(fe, x, scale=1.0):
    t = torch.from_numpy(x).to("cuda:0")
    return (fe(t, scale=scale) if x.dtype == np.int16 else fe(t)).cpu().numpy()


@pytest.mark.parametrize("db", pr.LEVELS_FLOAT)
@pytest.mark.parametrize("layout", pr.LAYOUTS)
@pytest.mark.parametrize("form", list(FORMS))
def test_quiet_frame_next_to_a_loud_one(level_front_ends, form, layout, db):
    """A quiet frame (scaled speech-like content with weak high bands, and white noise) and a loud one `db` apart wherever a pair
    can form: a step inside a row behind an even and an odd frame and its mirror image, rows alternately loud and quiet with an
    odd frame count, a quiet row's zero-padded tail in front of a loud row."""
    fe, nfft = level_front_ends[form], FORMS[form][1].get("nfft", 512)
    for kind in pr.KINDS:
        case = pr.level_case(layout, db, kind)
        pr.check_level_case(case, _run(fe, case.x), _run(fe, case.flat), pr.level_oracle(layout, db, kind, nfft),
                            f"form {fe.kernel_form()}, {case.name}")


@pytest.mark.parametrize("scale", pr.PCM_SCALES)
@pytest.mark.parametrize("layout", pr.LAYOUTS)
@pytest.mark.parametrize("form", list(FORMS))
def test_lsb_noise_next_to_full_scale_speech_in_pcm(level_front_ends, form, layout, scale):
    """16-bit PCM: integer noise of +-1..3 LSB beside speech that peaks near 30 000 (80 dB), converted inside the kernel; and bit
    for bit what the float path gives for the converted samples."""
    fe, nfft = level_front_ends[form], FORMS[form][1].get("nfft", 512)
    case = pr.level_case(layout, 0, "pcm")
    assert case.x.dtype == np.int16 and np.abs(case.x).max() > 29000
    got = _run(fe, case.x, scale)
    pr.check_level_case(case, got, _run(fe, case.flat, scale), pr.level_oracle(layout, 0, "pcm", nfft, scale),
                        f"form {fe.kernel_form()}, scale {scale:.3g}, {case.name}")
    assert np.array_equal(got, _run(fe, pr.as_float(case.x, scale)))


@pytest.mark.parametrize("form", list(FORMS))
def test_silent_frame_behind_an_even_and_an_odd_live_frame(level_front_ends, form):
    """The exact-zero rule in every form and at both parities: digital silence that begins at sample 160 f + 400 (f = 4, 5) makes
    frame f + 3 the first all-zero one, paired with a live frame for one of the two f in either kernel; it comes out as the
    package's log(eps), not as the log of its partner's rounding noise (about -30)."""
    from conftest import assert_parity
    fe, nfft = level_front_ends[form], FORMS[form][1].get("nfft", 512)
    x = np.stack([pr._speechlike(2000, 700 + r) for r in range(4)])
    x[0, 1040:] = x[1, 1200:] = 0.0
    x[2, :1040] = x[3, :1200] = 0.0                               # and silence in front of a live frame
    ref = pr.oracle_rows(x, **{**pr.REFERENCE_CALL, "nfft": nfft})
    silent = np.isclose(ref[..., 0], np.log(np.finfo(float).eps))
    assert [int(silent[r].sum()) for r in range(4)] == [4, 3, 5, 6]
    got = _run(fe, x)
    assert np.abs(got[silent] - ref[silent]).max() <= 1e-3        # (-36.04 and 23 zeros; the partner's noise would be off by 6)
    assert_parity(got, ref, 1e-4, f"form {fe.kernel_form()}, silence next to live frames", elem_tol=1e-3)


@pytest.mark.parametrize("plan,form", LOGMEL_FORMS)
def test_tones_band_by_band(plan, form):
    """A tone in every bin (and 0.37 bins off it), one frame per row, all rows in one launch: every band's log energy in every
    row against the oracle's."""
    kw = pr.LOGMEL_PLANS[plan]
    fe = _front_end(form, **kw)
    rows, _ = pr.tone_rows(kw["nfft"])
    ref, bar, own = pr.logmel_bar(rows, kw)
    pr.log_figures(f"[logmel] fp32 reference, {plan}, tones: worst {own:.3e}")
    got = _run(fe, rows)
    assert got.shape == (kw["nfft"] + 1, 1, kw["nfilt"])
    pr.check_logmel(got, ref, bar, f"form {fe.kernel_form()}, {plan}, tones")


@pytest.mark.parametrize("plan,form", LOGMEL_FORMS)
def test_frame_edges_band_by_band(plan, form):
    """A unit impulse on a frame's last sample and on the first sample outside it, behind an even and an odd frame: the frame's
    bands say whether the kernel read it."""
    kw = pr.LOGMEL_PLANS[plan]
    fe = _front_end(form, **kw)
    rows, _ = pr.edge_rows()
    ref, bar, own = pr.logmel_bar(rows, kw)
    pr.log_figures(f"[logmel] fp32 reference, {plan}, edges: worst {own:.3e}")
    pr.check_logmel(_run(fe, rows), ref, bar, f"form {fe.kernel_form()}, {plan}, edges")
