"""Probes of the MFCC kernels (csrc/mfcc.hip) and their CPU references.  TEST INFRASTRUCTURE ONLY.

The kernels transform two frames as one complex signal and split the spectra afterwards; in fp32 the split hands each frame
the other frame's rounding noise.  Two kinds of input make that, and a misplaced bin or weight, visible:

  * LEVEL STEPS inside a pair (`step_rows`, `alternating_rows`, `padded_tail_rows`): a quiet part (never exactly zero) and a
    loud part, 0 to 160 dB apart, laid out so that every place where two frames can be paired -- inside a row, across two
    rows of a batch, at the zero-padded tail of a row -- has a quiet frame next to a loud one at both parities.  With the
    inputs come boolean masks of the frames that are entirely quiet and entirely loud, and the same input with the loud part
    at the quiet level (`flat`): a quiet frame's result must not depend on its neighbour.
  * TONES and FRAME EDGES (`tone_rows`, `edge_rows`), looked at band by band: with numcep = nfilt and no lifter the orthonormal
    DCT is inverted by one transpose product (`logmel_from_cepstra`), so the output IS the log-mel spectrum.

`mfcc_fp32_unpaired` is the oracle's chain in float32 with one real transform per frame: what a correct fp32 kernel without
pairing computes.  tests/test_mfcc_probes.py shows on the CPU that it alone meets every bar the GPU tests apply
(`check_level_case`, `check_logmel` -- the same functions run on the kernel's output), and that a spectrum displaced by one
bin or one filterbank weight off by 1 % does not.
"""
from __future__ import annotations

import functools
import os
from typing import NamedTuple

import numpy as np
import scipy.fft

import mfcc_oracle as mo
from test_mfcc import _speechlike

REFERENCE_CALL = dict(numcep=24, nfilt=26, nfft=512)          # reference dataset.py:128
LEVELS_FLOAT = (0, 40, 60, 80, 90, 120, 160)                  # dB between the loud part (peak near 1.0) and the quiet part
KINDS = ("speech", "white")                                   # quiet content: scaled _speechlike (weak high bands), white noise
LAYOUTS = ("step", "rows_loud_first", "rows_quiet_first", "tail")
PCM_SCALES = (1.0, 1.0 / 32768)
FRAME_LEN, FRAME_STEP = 400, 160                              # 25 ms / 10 ms at 16 kHz
# band-by-band plans: numcep = nfilt, no lifter, c0 kept (the inversion needs all of the DCT's rows)
LOGMEL = dict(ceplifter=0, appendEnergy=False)
LOGMEL_PLANS = {"ref512": dict(nfft=512, nfilt=26, numcep=26, **LOGMEL),
                "tel512": dict(nfft=512, nfilt=20, numcep=20, lowfreq=300, highfreq=3400, **LOGMEL),
                "gen1024": dict(nfft=1024, nfilt=26, numcep=26, **LOGMEL)}


# ---- references -----------------------------------------------------------------------------------------------------

def dct_matrix(n, ncoef=None):
    """Orthonormal DCT-II, [ncoef, n] float64: mfcc_oracle.dct2_ortho(x, ncoef) == x @ dct_matrix(n, ncoef).T."""
    ncoef = n if ncoef is None else ncoef
    k, m = np.arange(ncoef)[:, None], np.arange(n)[None, :]
    d = np.cos(np.pi * k * (2 * m + 1) / (2.0 * n)) * np.sqrt(2.0 / n)
    d[0] *= np.sqrt(0.5)
    return d


def logmel_from_cepstra(c):
    """[..., n] unliftered cepstra of n filters (numcep = nfilt) -> [..., n] log mel energies, float64: D is orthonormal, so
    c = logmel @ D.T is inverted by c @ D."""
    c = np.asarray(c, dtype=np.float64)
    return c @ dct_matrix(c.shape[-1])


def mfcc_fp32_unpaired(x, samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=26, nfft=512, lowfreq=0, highfreq=None,
                       preemph=0.97, ceplifter=22, appendEnergy=True, roll_bins=0, fb=None):
    """mfcc_oracle.mfcc with float32 arithmetic throughout and one real transform per frame (scipy.fft.rfft of float32 stays
    complex64): no pairing, so no frame sees another's rounding noise.  `roll_bins`, `fb`: deliberate defects for the CPU test
    of the tone probe -- the spectrum displaced by that many bins, another filterbank matrix [nfilt, nfft/2 + 1]."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    y = np.concatenate([x[:1], x[1:] - f32(preemph) * x[:-1]]).astype(f32)
    frames = mo.framesig(y, winlen * samplerate, winstep * samplerate).astype(f32)       # (zero padding only: exact)
    spec = scipy.fft.rfft(frames, nfft, axis=1)
    assert spec.dtype == np.complex64
    if roll_bins:
        spec = np.roll(spec, roll_bins, axis=1)
    p = (spec.real * spec.real + spec.imag * spec.imag) * f32(1.0 / nfft)
    eps = f32(np.finfo(float).eps)
    energy = p.sum(axis=1, dtype=f32)
    energy = np.where(energy == 0, eps, energy)
    if fb is None:
        fb = mo.get_filterbanks(nfilt, nfft, samplerate, lowfreq, highfreq or samplerate / 2)
    feat = p @ np.asarray(fb, dtype=f32).T
    feat = np.log(np.where(feat == 0, eps, feat))
    feat = feat @ dct_matrix(nfilt, numcep).astype(f32).T
    if ceplifter > 0:
        feat = feat * mo.lifter_coeffs(numcep, ceplifter).astype(f32)
    if appendEnergy:
        feat[:, 0] = np.log(energy)
    assert feat.dtype == f32
    return feat


def oracle_rows(waves, **kw):
    return np.stack([mo.mfcc(w, 16000, **kw) for w in waves])


def fp32_rows(waves, **kw):
    return np.stack([mfcc_fp32_unpaired(w, 16000, **kw) for w in waves])


def oracle_logmel_rows(waves, nfft, nfilt, lowfreq=0, highfreq=None, **_):
    return np.stack([np.log(mo.fbank(np.asarray(w, np.float64), 16000, nfilt=nfilt, nfft=nfft, lowfreq=lowfreq, highfreq=highfreq)[0])
                     for w in waves])


def as_float(x, scale=1.0):
    """What the kernel makes of 16-bit PCM: (float)s * scale, one fp32 rounding."""
    return x if x.dtype == np.float32 else x.astype(np.float32) * np.float32(scale)


def rowwise_rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-30)


def log_figures(line):
    """Figures of a run go to stdout and, with XVEC_PROBE_LOG set, into that file (profiles/mfcc_probe_errors.txt is made of
    such logs)."""
    print(line)
    if os.environ.get("XVEC_PROBE_LOG"):
        with open(os.environ["XVEC_PROBE_LOG"], "a") as f:
            f.write(line + "\n")


# ---- level steps inside a pair --------------------------------------------------------------------------------------

class LevelCase(NamedTuple):
    name: str
    x: np.ndarray          # [B, n] float32, or int16 PCM
    flat: np.ndarray       # the same with the loud part replaced by content at the quiet level
    quiet: np.ndarray      # [B, frames] bool: every sample the frame reads is quiet
    loud: np.ndarray       # [B, frames] bool: every sample the frame reads is loud


def frame_span(f, n):
    """Samples frame f of an n-sample row reads: its own and, for the pre-emphasis, the one before its first."""
    return max(FRAME_STEP * f - 1, 0), min(FRAME_STEP * f + FRAME_LEN, n)


def _masks(is_loud):
    B, n = is_loud.shape
    F = mo.num_frames(n)
    quiet, loud = np.zeros((B, F), bool), np.zeros((B, F), bool)
    for f in range(F):
        lo, hi = frame_span(f, n)
        quiet[:, f] = ~is_loud[:, lo:hi].any(axis=1)
        loud[:, f] = is_loud[:, lo:hi].all(axis=1)
    return quiet, loud


def quiet_factor(db):
    return 10.0 ** (-db / 20.0)


def _contents(B, n, db, kind, seed):
    """(loud, quiet, loud content at the quiet level), each [B, n]: float32 with the loud peak at 1.0, or for kind 'pcm' int16
    with the loud peak at 30 000 and integer noise of +-1..3 LSB as the quiet part."""
    rng = np.random.default_rng(seed)
    loud = np.stack([_speechlike(n, seed + 1 + i) for i in range(B)])
    if kind == "pcm":
        def lsb():
            return (rng.integers(1, 4, (B, n)) * rng.choice([-1, 1], (B, n))).astype(np.int16)
        return np.round(loud * 30000.0).astype(np.int16), lsb(), lsb()
    if kind == "speech":
        quiet = np.stack([_speechlike(n, seed + 101 + i) for i in range(B)])
    else:
        quiet = rng.standard_normal((B, n))
        quiet = quiet / np.abs(quiet).max(axis=1, keepdims=True)
    q = np.float32(quiet_factor(db))
    return loud, (quiet * q).astype(np.float32), (loud * q).astype(np.float32)


def _case(name, is_loud, db, kind, seed):
    loud, quiet, loud_down = _contents(*is_loud.shape, db, kind, seed)
    x, flat = np.where(is_loud, loud, quiet), np.where(is_loud, loud_down, quiet)
    assert (x[~is_loud] != 0).all() and (flat != 0).all()     # quiet is never silent: exact zeros have a code path of their own
    return LevelCase(name, x, flat, *_masks(is_loud))


@functools.lru_cache(maxsize=None)
def step_rows(db, kind):
    """A step inside a row: 2000 samples (11 frames), quiet then loud with the step at sample 160 f + 400 for f = 4 and 5 --
    frame f is the last all-quiet one, frame f + 1 holds loud samples, and f is even once and odd once, whichever way a kernel
    numbers its pairs -- and the mirror image, loud then quiet, at the same two steps."""
    n = 2000
    is_loud = np.zeros((4, n), bool)
    for r, (f, loud_first) in enumerate([(4, False), (5, False), (4, True), (5, True)]):
        s = FRAME_STEP * f + FRAME_LEN
        is_loud[r, :s] = loud_first
        is_loud[r, s:] = not loud_first
    return _case(f"step {db} dB {kind}", is_loud, db, kind, 1000 + db)


@functools.lru_cache(maxsize=None)
def alternating_rows(db, kind, loud_first):
    """Across rows: eight rows of 720 samples (3 frames: odd, so the nfft-512 kernel pairs a row's last frame with the next row's
    first), alternately all loud and all quiet."""
    is_loud = np.zeros((8, 720), bool)
    is_loud[(0 if loud_first else 1)::2] = True
    return _case(f"rows {'loud' if loud_first else 'quiet'} first {db} dB {kind}", is_loud, db, kind, 2000 + db)


@functools.lru_cache(maxsize=None)
def padded_tail_rows(db, kind):
    """The zero-padded tail: rows of 1999 samples (11 frames; the last one reads 399 samples and one of padding), quiet, loud,
    loud, quiet, loud -- a quiet row's tail frame is paired with a loud row's first frame and a quiet row's first frame with a
    loud row's tail, at both parities of the batch's frame numbering (n = 1999 of the three sizes the issue offers: the
    cheapest with an odd frame count)."""
    is_loud = np.zeros((5, 1999), bool)
    is_loud[[1, 2, 4]] = True
    return _case(f"tail {db} dB {kind}", is_loud, db, kind, 3000 + db)


def level_case(layout, db, kind):
    if layout == "step":
        return step_rows(db, kind)
    if layout == "tail":
        return padded_tail_rows(db, kind)
    return alternating_rows(db, kind, layout == "rows_loud_first")


@functools.lru_cache(maxsize=None)
def level_oracle(layout, db, kind, nfft, scale=1.0):
    return oracle_rows(as_float(level_case(layout, db, kind).x, scale), **{**REFERENCE_CALL, "nfft": nfft})


def check_level_case(case, got, got_flat, ref, what):
    """The bars of the level tests on one output [B, frames, numcep] (a kernel's, or the fp32 reference's): the path's own bar
    (assert_parity 1e-4 row-wise, 1e-3 element-wise) on the all-quiet frames ALONE -- the element-wise bound's absolute part is
    scaled by mean |ref| of what it is given --, on the all-loud frames alone, and on everything; and the quiet frames equal to
    those of the run with the loud part at the quiet level inside 1e-5 row-wise (README: batch composition).  Returns the figures."""
    from conftest import assert_parity
    got, got_flat = np.asarray(got, np.float64), np.asarray(got_flat, np.float64)
    quiet, loud = case.quiet, case.loud
    assert quiet.shape == loud.shape == got.shape[:2] == ref.shape[:2]
    mixed = ~quiet & ~loud
    assert not (quiet & loud).any() and (quiet | loud | mixed).all()          # the three masks leave no frame out
    assert quiet.sum() >= 4 and loud.sum() >= 4, (what, int(quiet.sum()), int(loud.sum()))
    fig = dict(quiet=rowwise_rel(got[quiet], ref[quiet]).max(), loud=rowwise_rel(got[loud], ref[loud]).max(),
               mixed=rowwise_rel(got[mixed], ref[mixed]).max() if mixed.any() else 0.0,
               c0_loud=np.abs(got[loud][:, 0] - ref[loud][:, 0]).max(), c0_quiet=np.abs(got[quiet][:, 0] - ref[quiet][:, 0]).max(),
               neighbour=rowwise_rel(got[quiet], got_flat[quiet]).max())
    log_figures(f"[level] {what}: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert_parity(got[quiet], ref[quiet], 1e-4, f"{what}, quiet frames", elem_tol=1e-3)
    assert_parity(got[loud], ref[loud], 1e-4, f"{what}, loud frames", elem_tol=1e-3)
    assert_parity(got, ref, 1e-4, f"{what}, all frames", elem_tol=1e-3)
    assert fig["neighbour"] <= 1e-5, f"{what}: quiet frames move by {fig['neighbour']:.2e} row-wise with the neighbour's level"
    return fig


# ---- band by band: tones and frame edges ----------------------------------------------------------------------------

TONE_DELTA = 0.37


@functools.lru_cache(maxsize=None)
def tone_rows(nfft):
    """One-frame rows of 400 samples, 0.5 cos(2 pi (k + d) n / nfft + 0.3): every bin k = 0 .. nfft/2 with d = 0, then every
    bin below nfft/2 with d = 0.37 -- neighbouring rows (tones k and k + 1) share a transform in the nfft-512 kernel, at both
    parities.  Returns (rows [nfft + 1, 400] float32, the tones' bins k + d)."""
    bins = np.concatenate([np.arange(nfft // 2 + 1, dtype=np.float64), np.arange(nfft // 2) + TONE_DELTA])
    n = np.arange(FRAME_LEN)
    return (0.5 * np.cos(2 * np.pi * bins[:, None] * n[None, :] / nfft + 0.3)).astype(np.float32), bins


@functools.lru_cache(maxsize=None)
def edge_rows():
    """Rows of 2000 samples of 1e-3 noise with a unit impulse at the last sample of frame f (160 f + 399) and, in another row, at
    the first sample outside it (160 f + 400), for f = 4 and f = 5: whether frame f holds the impulse changes its energy by three
    orders of magnitude."""
    rng = np.random.default_rng(77)
    x = (1e-3 * rng.standard_normal((4, 2000))).astype(np.float32)
    at = [FRAME_STEP * f + FRAME_LEN - 1 + out for f in (4, 5) for out in (0, 1)]
    for r, s in enumerate(at):
        x[r, s] += 1.0
    return x, at


def logmel_bar(rows, plan):
    """(oracle log-mel [rows, frames, nfilt], bar): the bar is 8 x the largest absolute log-mel error of the fp32 reference on
    these rows, floor 1e-5 -- the 8 for what a kernel legitimately does differently (another factorisation in packed fp32, the
    mel product in another order, the 2^-6 pre-scaling); a displaced bin moves a band by 0.1 or more."""
    ref = oracle_logmel_rows(rows, **plan)
    own = np.abs(logmel_from_cepstra(fp32_rows(rows, **plan)) - ref).max()
    return ref, max(8.0 * own, 1e-5), own


def check_logmel(cep, ref, bar, what, widen=1.0):
    """Band by band and frame by frame: |log-mel of the output - oracle| <= bar.  Returns (worst error, its index)."""
    assert widen * bar <= 1e-3 or widen == 1.0
    err = np.abs(logmel_from_cepstra(cep) - ref)
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    log_figures(f"[logmel] {what}: worst {err.max():.3e} at (row, frame, band) {tuple(int(i) for i in at)}, bar {widen * bar:.3e}")
    assert np.isfinite(err).all() and err.max() <= widen * bar, \
        f"{what}: log-mel off by {err.max():.3e} at (row, frame, band) {tuple(int(i) for i in at)}, bar {widen * bar:.3e}"
    return err.max(), at
