"""include/xvec_vad.h restated in numpy: the energy VAD with the header's fixed order of the energy sum (an explicit loop, never
np.sum), an independent threshold from math.fsum, the window of a frame, and sliding CMVN with direct window sums in
np.longdouble.  Written from the header, which is the specification: parity with Kaldi itself is unpinned (not installed where
this was written).  A plain module like diar_ref.py; the test files import it."""
import math

import numpy as np

LANES = 256          # XVEC_VAD_LANES (tests/test_vad.py ties it to the header)
VAR_FLOOR = 1e-10

VAD_DEFAULTS = dict(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6, energy_col=0)
RECIPE_VAD = dict(energy_threshold=5.5, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.12)


# ---------------------------------------------------------------- energy VAD

def fixed_order_sum(e) -> np.float64:
    """The header's S of the fp32 energies e[0 .. L - 1]: LANES partial sums, partial j adding e[j], e[j + LANES], ... in
    ascending order, then the stride-halving tree."""
    e = np.asarray(e, dtype=np.float32)
    part = [np.float64(0.0)] * LANES
    for t in range(e.shape[0]):
        part[t % LANES] = np.float64(part[t % LANES] + np.float64(e[t]))
    stride = LANES // 2
    while stride >= 1:
        for j in range(stride):
            part[j] = np.float64(part[j] + part[j + stride])
        stride //= 2
    return part[0]


def threshold(e, energy_threshold=5.0, energy_mean_scale=0.5, **_) -> np.float64:
    """thr of the header: every operation rounded on its own; an empty utterance with a mean scale has NaN."""
    if energy_mean_scale == 0:
        return np.float64(energy_threshold)
    L = len(e)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(fixed_order_sum(e)) / np.float64(L)
        scaled = np.float64(energy_mean_scale) * mean
        return np.float64(np.float64(energy_threshold) + scaled)


def threshold_fsum(e, energy_threshold=5.0, energy_mean_scale=0.5, **_) -> float:
    """The same threshold from the correctly rounded sum: what the fixed order is held against."""
    if energy_mean_scale == 0:
        return float(energy_threshold)
    e = np.asarray(e, dtype=np.float32)
    return float(energy_threshold) + float(energy_mean_scale) * (math.fsum(float(v) for v in e) / len(e))


def decide(e, thr, frames_context=0, proportion_threshold=0.6, **_) -> np.ndarray:
    """uint8 [L]: the votes of the header on the fp32 energies e against the threshold thr."""
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    L = e.shape[0]
    with np.errstate(invalid="ignore"):
        hot = e > np.float64(thr)                 # NaN on either side: False
    csum = np.concatenate([[0], np.cumsum(hot)])
    t = np.arange(L)
    lo, hi = np.maximum(0, t - frames_context), np.minimum(L - 1, t + frames_context)
    num, den = csum[hi + 1] - csum[lo], hi + 1 - lo
    return (num.astype(np.float64) >= den.astype(np.float64) * np.float64(proportion_threshold)).astype(np.uint8)


def energy_vad(x, lengths=None, **opts):
    """(mask uint8 [B, T], counts int32 [B], thr float64 [B]) of x [B, T, C] float32."""
    o = {**VAD_DEFAULTS, **opts}
    B, T, _ = x.shape
    lengths = [T] * B if lengths is None else [int(v) for v in lengths]
    mask, thr = np.zeros((B, T), dtype=np.uint8), np.zeros(B, dtype=np.float64)
    for b, L in enumerate(lengths):
        e = x[b, :L, o["energy_col"]]
        thr[b] = threshold(e, **o)
        mask[b, :L] = decide(e, thr[b], **o)
    return mask, mask.sum(1).astype(np.int32), thr


# ---------------------------------------------------------------- sliding CMVN

def window(t, L, cmn_window, min_window, center):
    """[lo, hi) of frame t in an utterance of L frames."""
    if center:
        lo = t - cmn_window // 2
        hi = lo + cmn_window
    else:
        lo = t - cmn_window
        hi = t + 1
    if lo < 0:
        hi -= lo
        lo = 0
    if not center and hi > t:
        hi = max(t + 1, min_window)
    if hi > L:
        lo -= hi - L
        hi = L
        if lo < 0:
            lo = 0
    return lo, hi


def tile_plan(C, span, lanes=LANES, tile_max=256, tile_min=16, group_min=8, lds_bytes=61440):
    """(frames of a tile, channels of a group, frames of a run) of csrc/vad_plan.h for C channels and windows of at most
    `span` frames, or None where it refuses: the tallest tile whose rows fit the LDS budget, all channels before halves of
    them; as many runs as whole sets of the group's channels fit the block's lanes."""
    gmin = min(C, group_min)
    frames = tile_max
    while frames >= tile_min:
        rows, parts = frames - 1 + span, 1
        while True:
            ch = max(-(-C // parts), gmin)
            if rows * ch * 4 <= lds_bytes:
                runs = min(frames, max(1, lanes // ch))
                return frames, ch, -(-frames // runs)
            if ch == gmin:
                break
            parts *= 2
        frames //= 2
    return None


def span(cmn_window=600, min_window=100, center=False, **_):
    return cmn_window if center else max(cmn_window + 1, min_window)


def sliding_cmvn(x, cmn_window=600, min_window=100, center=False, norm_vars=False, tile=None, run=1):
    """One utterance x [L, C] float32 -> (y, bound), both np.longdouble [L, C]: the header's values with every window sum
    formed afresh in np.longdouble and NO final rounding to fp32, and the bound on |(float32 result of the header's fp64
    arithmetic) - y| (tests/test_vad_gpu.py derives it in its docstring).  `tile`, `run`: the header's F and R, which set
    how many fp64 operations a window's sums have been through; run = 1 is a sum formed afresh."""
    x = np.asarray(x, dtype=np.float32)
    L, C = x.shape
    xl = x.astype(np.longdouble)
    xa, xq = np.abs(xl), xl * xl
    y, bound = np.zeros((L, C), np.longdouble), np.zeros((L, C), np.longdouble)
    u = np.longdouble(2.0) ** -53 + np.finfo(np.longdouble).eps      # an fp64 rounding, and this restatement's own
    for t in range(L):
        lo, hi = window(t, L, cmn_window, min_window, center)
        n = hi - lo
        mean = xl[lo:hi].sum(0) / n
        # the run's first frame ts summed its window; every frame up to t added what entered and subtracted what left:
        # k operations in all, each rounding a partial sum of values of the rows [lo(ts), hi), none larger than their sum|x|
        ts = t if run == 1 else t // tile * tile + (t % tile) // run * run
        lo_s, hi_s = window(ts, L, cmn_window, min_window, center)
        k = (hi_s - lo_s) + (hi - hi_s) + (lo - lo_s)
        sabs = xa[lo_s:hi].sum(0)
        d = xl[t] - mean
        # the sums are off by at most k u sum|x|; the quotient adds u |mean|; the difference u |d|
        dmean = (k * u * sabs) / n + u * np.abs(mean)
        if not norm_vars:
            y[t] = d
            bound[t] = dmean + u * np.abs(d)
            continue
        if n == 1:
            continue                                                 # zeros, exactly
        sq = xq[lo:hi].sum(0)
        var = sq / n - mean * mean
        # sumsq: k u (the squares of the run's rows; those of fp32 values are exact in fp64); its quotient, the product
        # mean * mean (with the mean's own error) and the difference round once each at the size of their operands
        dvar = (k * u * xq[lo_s:hi].sum(0)) / n + u * (sq / n) + 2 * np.abs(mean) * dmean + dmean * dmean + u * mean * mean \
            + u * (sq / n + mean * mean)
        var_lo, var_hi = np.maximum(var - dvar, VAR_FLOOR), np.maximum(var + dvar, VAR_FLOOR)
        var = np.maximum(var, VAR_FLOOR)
        scale = 1 / np.sqrt(var)
        y[t] = d * scale
        # the scale anywhere in [var_hi^-1/2, var_lo^-1/2], three more fp64 roundings (sqrt, reciprocal, product)
        dscale = np.maximum(1 / np.sqrt(var_lo) - scale, scale - 1 / np.sqrt(var_hi)) + 3 * u * 1 / np.sqrt(var_lo)
        bound[t] = (np.abs(d) + dmean + u * np.abs(d)) * dscale + (dmean + u * np.abs(d)) * scale + u * np.abs(y[t])
    return y, bound


def select(rows, mask):
    """(out, new_len): the rows of one utterance [T, C] whose mask is set, in order, zeros behind."""
    keep = np.flatnonzero(np.asarray(mask) != 0)
    out = np.zeros_like(rows)
    out[:len(keep)] = rows[keep]
    return out, len(keep)
