"""Waveform augmentation restated in numpy float64 for arbitrary shapes: what the kernels of csrc/augment.hip are checked
against (include/xvec_augment.h states the arithmetic).  tests/test_augment.py pins this module to the reference's own run
(tests/golden/g9_augment.npz).  A plain module like eer_ref.py; the test files import it."""
import numpy as np

EPS = 1e-20      # the reference's EPS


def noise_of(op, srcs, pool, pool_len):
    """The op's summed noise, float64 [length]: the sources in list order, zeros past a clip's end."""
    z = None
    for k in range(int(op["first_src"]), int(op["first_src"]) + int(op["n_src"])):
        row, start = int(srcs[k]["row"]), int(srcs[k]["start"])
        one = np.zeros(int(op["length"]), dtype=np.float64)
        if 0 <= row < len(pool_len) and start >= 0:
            part = np.asarray(pool[row][start:min(int(pool_len[row]), start + int(op["length"]))], dtype=np.float64)
            one[:part.size] = part
        z = one if z is None else z + one
    return np.zeros(int(op["length"])) if z is None else z


def mix(waves, pool, pool_len, ops, srcs):
    """(float64 [B, n] result, float64 gains [n_ops]); the ops of an utterance in list order, each on the result of the last."""
    out = np.array(waves, dtype=np.float64)
    gains = np.zeros(len(ops))
    for o, op in enumerate(ops):
        sl = slice(int(op["offset"]), int(op["offset"]) + int(op["length"]))
        s = out[int(op["utt"]), sl].astype("int64")
        z = noise_of(op, srcs, pool, pool_len).astype("int64")
        s_rms = np.sqrt(np.mean(s ** 2))
        z_rms = np.sqrt(np.mean(z ** 2))
        w = np.sqrt(s_rms ** 2 / float(op["snr_ratio"]))
        out[int(op["utt"]), sl] = s + z * w / (z_rms + EPS)
        gains[o] = w / (z_rms + EPS)
    return out, gains


def conv_full(x, h):
    """Direct float64 convolution, n + L - 1 outputs."""
    return np.convolve(np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64))


def reverb_row(x, h, fft=False):
    """One utterance in the reference's order of operations (dataset.py:388-395); float64.  `fft` convolves as the
    reference does, scipy's fftconvolve with `h` in the dtype it has: a float32 response is transformed in SINGLE precision
    there (scipy.fft keeps the input's precision), so the reference itself is some 1e-8 of the peak away from the exact
    convolution, which is what fft=False computes and what the kernels are held to."""
    x = np.asarray(x, dtype=np.float64)
    if fft:
        from scipy.signal import fftconvolve
        c = fftconvolve(x, np.asarray(h))
    else:
        c = conv_full(x, h)
    c = c / np.abs(c).max()
    c = c * (np.abs(x).max() / np.abs(c).max())
    return x + c[:x.size]


def reverb(waves, rirs, rir_len, rir_index, fft=False):
    out = np.array(waves, dtype=np.float64)
    for b, r in enumerate(rir_index):
        if r >= 0:
            out[b] = reverb_row(out[b], rirs[r][:int(rir_len[r])], fft)
    return out


def reverb_bound(x, h):
    """Per-sample error bound of the fp32 kernel against `reverb_row`, derived (tests/test_augment_gpu.py):
       convolution   |c_got - c| <= (K + 8) 2^-24 (|x| * |h|), K taps: an fp32 sum of K exact products in any order
       scale         s = max|x| / max|c|: the peak inherits the bound at its own position, the quotient adds one rounding
       add           c s and x + c s: two roundings, covered by 2^-22 |ref|."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, K = x.size, h.size
    c = conv_full(x, h)
    e = (K + 8) * 2.0 ** -24 * conv_full(np.abs(x), np.abs(h))
    peak = np.abs(c).max()
    s = np.abs(x).max() / peak
    rel_s = e.max() / (peak - e.max()) + 2.0 ** -23          # any |c_got| peak lies within e.max() of the true peak
    ref = x + c[:n] * s
    return e[:n] * s * (1 + rel_s) + np.abs(c[:n]) * s * rel_s + 2.0 ** -22 * np.abs(ref), ref


def normalize(waves):
    out = np.array(waves, dtype=np.float64)
    out = out - out.min(axis=-1, keepdims=True)
    return out / out.max(axis=-1, keepdims=True)
