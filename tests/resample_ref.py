"""resampy 0.3.0's sinc resampling (resample_f, filter tables of sinc_window), RESTATED in numpy float64: the reference the
resampling kernel (include/xvec_resample.h) is checked against, bit for bit.  resampy itself is not installed where this was
written, so parity with the package is unpinned; the algorithm is the one in the header's comment.

Three forms of the same arithmetic: `tap_plan` (one output's centre, table offsets, interpolation weights and tap counts),
`resample_loops` (the literal double loop, for tiny inputs) and `resample` (vectorised over the outputs of a row with the tap
index as the outer loop: every output still adds its taps in the package's order, left wing first).  numpy evaluates a + b * c as
two ufuncs, each rounded on its own: nothing here is fused.  A plain module like snorm_ref.py and lda_ref.py."""
import numpy as np

KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492)
KAISER_FAST = dict(num_zeros=16, precision=9, rolloff=0.85, beta=8.555504641634386)


def sinc_window(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596):
    m = (2 ** precision) * num_zeros
    return rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, m + 1)) * np.kaiser(2 * m + 1, beta)[m:]


def ratio_plan(ratio, precision):
    """(inc, scale, step) of a ratio."""
    ratio = float(ratio)
    scale = min(1.0, ratio)
    return 1.0 / ratio, scale, int(scale * (2 ** precision))


def num_out(n, ratio):
    return int(n * float(ratio))


def tap_plan(t, ratio, precision, nwin, n):
    """(n0, off_l, eta_l, i_max, off_r, eta_r, k_max) of output t of a row of n samples, in Python floats (IEEE doubles)."""
    P = 2 ** precision
    inc, scale, step = ratio_plan(ratio, precision)
    time = t * inc
    n0 = int(time)
    frac = scale * (time - n0)
    idx = frac * P
    off_l = int(idx)
    eta_l = idx - off_l
    i_max = min(n0 + 1, (nwin - off_l) // step)
    frac = scale - frac
    idx = frac * P
    off_r = int(idx)
    eta_r = idx - off_r
    k_max = min(n - n0 - 1, (nwin - off_r) // step)
    return n0, off_l, eta_l, i_max, off_r, eta_r, k_max


def _scaled_table(win, ratio):
    win = np.asarray(win, dtype=np.float64)
    win_s = win * float(ratio) if float(ratio) < 1 else win.copy()
    delta = np.zeros_like(win_s)
    delta[:-1] = win_s[1:] - win_s[:-1]
    return win_s, delta


def resample_loops(x, ratio, win, precision, accumulate="float64"):
    """One row, the literal double loop.  float64 output; with accumulate='float32' the running sum is rounded to float32 after
    every tap (every value of the output is then a float32)."""
    x = np.asarray(x).astype(np.float64)
    n, nwin = x.shape[0], len(win)
    win_s, delta = _scaled_table(win, ratio)
    _, _, step = ratio_plan(ratio, precision)
    f32 = accumulate == "float32"
    y = np.zeros(num_out(n, ratio), dtype=np.float64)
    for t in range(y.shape[0]):
        n0, off_l, eta_l, i_max, off_r, eta_r, k_max = tap_plan(t, ratio, precision, nwin, n)
        acc = 0.0
        for i in range(i_max):
            w = float(win_s[off_l + i * step]) + eta_l * float(delta[off_l + i * step])
            acc = acc + w * float(x[n0 - i])
            if f32:
                acc = float(np.float32(acc))
        for k in range(k_max):
            w = float(win_s[off_r + k * step]) + eta_r * float(delta[off_r + k * step])
            acc = acc + w * float(x[n0 + k + 1])
            if f32:
                acc = float(np.float32(acc))
        y[t] = acc
    return y


def resample_row(x, ratio, win, precision, accumulate="float64"):
    """One row, vectorised over its outputs; the same bits as resample_loops."""
    x = np.asarray(x).astype(np.float64)
    n, nwin, P = x.shape[0], len(win), 2 ** precision
    win_s, delta = _scaled_table(win, ratio)
    inc, scale, step = ratio_plan(ratio, precision)
    f32 = accumulate == "float32"
    n_out = num_out(n, ratio)
    y = np.zeros(n_out, dtype=np.float64)
    if n_out == 0:
        return y
    time = np.arange(n_out, dtype=np.float64) * inc
    n0 = time.astype(np.int64)
    frac = scale * (time - n0)
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        idx = frac * P
        off = idx.astype(np.int64)
        eta = idx - off
        count = np.minimum(n - n0 - 1 if wing else n0 + 1, (nwin - off) // step)
        for i in range(int(count.max(initial=0))):
            m = i < count
            j = off[m] + i * step
            w = win_s[j] + eta[m] * delta[j]
            acc = y[m] + w * x[n0[m] + i + 1 if wing else n0[m] - i]
            y[m] = acc.astype(np.float32).astype(np.float64) if f32 else acc
    return y


def resample(x, ratios, win, precision, accumulate="float64", lens=None):
    """x [B, n] (or [n]); row b at ratios[b] (a scalar serves all rows) over its first lens[b] samples.  Returns
    (out float64 [B, max(1, longest output)] zero past out_lens[b], out_lens int64 [B])."""
    x = np.atleast_2d(np.asarray(x))
    B, n = x.shape
    ratios = np.broadcast_to(np.atleast_1d(np.asarray(ratios, dtype=np.float64)), (B,))
    lens = np.full(B, n, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)
    rows = [resample_row(x[b, :lens[b]], ratios[b], win, precision, accumulate) for b in range(B)]
    out = np.zeros((B, max(1, max(num_out(n, r) for r in ratios))), dtype=np.float64)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out, np.array([r.shape[0] for r in rows], dtype=np.int64)
