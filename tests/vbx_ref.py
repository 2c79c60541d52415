"""VBx in numpy, the oracle of include/xvec_vbx.h (tests/test_vbx.py holds its two forms against each other, tests/test_vbx_gpu.py
the kernels against them).  A plain module like diar_ref.py; the test files import it.

  vbx_log      the log-domain form, written as the header's specification reads: the dense transition matrix, scipy's
               logsumexp per frame.  O(T S^2).
  vbx_scaled   the scaled form the kernel runs: b_t = exp(logp_t - max_t), one sum over the speakers per frame and direction.
Both take a `dtype` (np.float64 or np.longdouble) and return (gamma [T, S], pi [S], elbo [max_iter] with NaN in the slots not
run, iters).  `labels_of` is the header's labelling rule, `init_gamma` xvec_vbx_init, `planted` / `noisy_labels` the test data.
"""
import math

import numpy as np
from scipy.special import logsumexp


def _constants(X, phi, dtype):
    D = X.shape[1]
    G = -0.5 * ((X ** 2).sum(axis=1, keepdims=True) + D * np.log(2 * dtype(np.pi)))
    rho = X * np.sqrt(phi)
    return G, rho


def _speaker_models(gamma, rho, phi, G, Fa, Fb):
    invL = 1.0 / (1 + Fa / Fb * gamma.sum(axis=0, keepdims=True).T * phi)
    alpha = Fa / Fb * invL * gamma.T.dot(rho)
    logp = Fa * (rho.dot(alpha.T) - 0.5 * (invL + alpha ** 2).dot(phi) + G)
    prior = Fb * 0.5 * np.sum(np.log(invL) - invL - alpha ** 2 + 1)
    return logp, prior


def _args(X, phi, gamma, pi, dtype):
    X = np.asarray(X, dtype=dtype)
    phi = np.asarray(phi, dtype=dtype)
    gamma = np.array(gamma, dtype=dtype)
    pi = np.array(pi, dtype=dtype)
    return X, phi, gamma, pi


def vbx_log(X, phi, gamma, pi, loop_prob=0.99, Fa=0.3, Fb=17.0, max_iter=40, epsilon=1e-4, dtype=np.float64):
    X, phi, gamma, pi = _args(X, phi, gamma, pi, dtype)
    loop_prob, Fa, Fb = dtype(loop_prob), dtype(Fa), dtype(Fb)
    T, S = gamma.shape
    G, rho = _constants(X, phi, dtype)
    elbo = np.full(max_iter, np.nan, dtype=dtype)
    iters = 0
    for k in range(max_iter):
        logp, prior = _speaker_models(gamma, rho, phi, G, Fa, Fb)
        with np.errstate(divide="ignore"):
            ltr = np.log(np.eye(S, dtype=dtype) * loop_prob + (1 - loop_prob) * pi)
            lfw = np.full((T, S), -np.inf, dtype=dtype)
            lbw = np.full((T, S), -np.inf, dtype=dtype)
            lfw[0] = logp[0] + np.log(pi)
        lbw[-1] = 0.0
        for t in range(1, T):
            lfw[t] = logp[t] + logsumexp(lfw[t - 1] + ltr.T, axis=1)
        for t in reversed(range(T - 1)):
            lbw[t] = logsumexp(ltr + logp[t + 1] + lbw[t + 1], axis=1)
        tll = logsumexp(lfw[-1])
        gamma = np.exp(lfw + lbw - tll)
        elbo[k] = tll + prior
        arrive = np.exp(logsumexp(lfw[:-1], axis=1, keepdims=True) + logp[1:] + lbw[1:] - tll).sum(axis=0) if T > 1 else 0.0
        pi = gamma[0] + (1 - loop_prob) * pi * arrive
        pi = pi / pi.sum()
        iters = k + 1
        if k > 0 and elbo[k] - elbo[k - 1] < epsilon:
            break
    return gamma, pi, elbo, iters


def vbx_scaled(X, phi, gamma, pi, loop_prob=0.99, Fa=0.3, Fb=17.0, max_iter=40, epsilon=1e-4, dtype=np.float64):
    X, phi, gamma, pi = _args(X, phi, gamma, pi, dtype)
    loop_prob, Fa, Fb = dtype(loop_prob), dtype(Fa), dtype(Fb)
    T, S = gamma.shape
    G, rho = _constants(X, phi, dtype)
    elbo = np.full(max_iter, np.nan, dtype=dtype)
    iters = 0
    for k in range(max_iter):
        logp, prior = _speaker_models(gamma, rho, phi, G, Fa, Fb)
        live = pi != 0
        mx = logp[:, live].max(axis=1, keepdims=True)
        b = np.where(live, np.exp(logp - mx), 0.0).astype(dtype)
        q = (1 - loop_prob) * pi
        a = np.empty((T, S), dtype=dtype)
        c = np.empty(T, dtype=dtype)
        v = pi * b[0]
        for t in range(T):
            if t:
                v = (loop_prob * a[t - 1] + q * a[t - 1].sum()) * b[t]
            c[t] = v.sum()
            a[t] = v / c[t]
        gamma = np.empty((T, S), dtype=dtype)
        beta = np.ones(S, dtype=dtype)
        arrive = np.zeros(S, dtype=dtype)
        for t in range(T - 1, -1, -1):
            gamma[t] = a[t] * beta
            if t:
                w = b[t] * beta
                arrive += a[t - 1].sum() * q * w / c[t]
                beta = (loop_prob * w + (q * w).sum()) / c[t]
        elbo[k] = (np.log(c) + mx[:, 0]).sum() + prior
        pi = gamma[0] + arrive
        pi = pi / pi.sum()
        iters = k + 1
        if k > 0 and elbo[k] - elbo[k - 1] < epsilon:
            break
    return gamma, pi, elbo, iters


def labels_of(gamma):
    """(labels [T] int32, n_speakers): argmax over the speakers, ties to the lowest, renumbered in the order of first appearance."""
    raw = np.argmax(gamma, axis=1)
    _, first, inverse = np.unique(raw, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse.reshape(-1)].astype(np.int32), len(first)


def init_gamma(labels, n_spk, smoothing=5.0):
    """xvec_vbx_init: e / (e + (n_spk - 1)) at the label and 1 / (e + (n_spk - 1)) elsewhere, e = exp(smoothing) of the C
    library (math.exp); a label outside 0 .. n_spk - 1 gives the uniform row.  Returns (gamma [N, n_spk], the uniform prior)."""
    labels = np.asarray(labels)
    e = math.exp(smoothing)
    rest = e + float(n_spk - 1)
    g = np.full((labels.shape[0], n_spk), 1.0 / rest)
    known = (labels >= 0) & (labels < n_spk)
    g[np.flatnonzero(known), labels[known]] = e / rest
    g[~known] = 1.0 / float(n_spk)
    return g, np.full(n_spk, 1.0 / float(n_spk))


def planted(T, D, K, seed, sep=1.0):
    """(X [T, D], phi [D], speaker of every frame [T]): K speakers drawn from N(0, sep^2 diag(phi)), turns of 3 .. 11 frames,
    unit within-speaker noise."""
    rng = np.random.default_rng(seed)
    phi = np.sort(rng.uniform(0.5, 8.0, D))[::-1].copy()
    means = sep * rng.standard_normal((K, D)) * np.sqrt(phi)
    spk = np.empty(T, dtype=np.int64)
    t, cur = 0, int(rng.integers(K))
    while t < T:
        n = int(rng.integers(3, 12))
        spk[t:t + n] = cur
        t += n
        if K > 1:
            cur = (cur + 1 + int(rng.integers(K - 1))) % K
    X = means[spk] + rng.standard_normal((T, D))
    return X, phi, spk


def noisy_labels(spk, n_spk, seed, redraw=0.2):
    """The AHC-like init: the planted labels with a fifth of them redrawn among the n_spk speakers."""
    rng = np.random.default_rng(seed + 1000)
    lab = np.asarray(spk).copy() % n_spk
    flip = rng.random(lab.shape[0]) < redraw
    lab[flip] = rng.integers(0, n_spk, int(flip.sum()))
    return lab.astype(np.int32)


# ---------------------------------------------------------------- the cases tests/test_vbx.py and tests/test_vbx_gpu.py share

THREADS, PREFETCH, MAX_FRAMES = 256, 8, 16384         # tests/test_vbx.py ties them to include/xvec_vbx.h
OPTS = dict(loop_prob=0.99, Fa=0.3, Fb=17.0)

# name -> (T, D, S, planted speakers, seed, separation, iterations)
CASES = {}
for _T in (1, 2, 3, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1, PREFETCH - 1, PREFETCH + 1):
    CASES[f"T{_T}"] = (_T, 12, 5, 3, 100 + _T, 1.0, 10)
for _S in (1, 2, 15, 16, 17, 63, 64):
    CASES[f"S{_S}"] = (70, 8, _S, min(_S, 4), 200 + _S, 1.0, 10)
for _D in (1, 3, 4, 5, 16, 17, 130):
    CASES[f"D{_D}"] = (70, _D, 4, 3, 300 + _D, 1.0, 10)
CASES["issue65"] = (65, 16, 6, 4, 401, 1.0, 10)
CASES["issue257"] = (257, 32, 10, 6, 402, 1.0, 10)
CASES["issue513"] = (513, 128, 16, 8, 403, 1.0, 10)
CASES["cap"] = (MAX_FRAMES, 8, 4, 3, 404, 1.0, 2)
# The stop-rule cases, run again with epsilon = 1e-4 and up to 40 iterations.  Every ELBO increment of theirs is further than
# 1e-6 |ELBO| from epsilon (tests/test_vbx.py), which at epsilon = 1e-4 only a recording with |ELBO| < 100 can meet on the
# increment that stops it: few frames, few dimensions.
CASES["stop24"] = (24, 3, 4, 2, 662, 1.0, 10)
CASES["stop12"] = (12, 2, 3, 2, 627, 1.0, 10)
CASES["stop16"] = (16, 1, 3, 2, 668, 1.0, 10)
STOP_CASES = ("stop24", "stop12", "stop16")

_DATA, _REFS = {}, {}


def case_data(name):
    """(X, phi, gamma0, pi0) of a case: planted speakers, the AHC-like noisy init with smoothing 5."""
    if name not in _DATA:
        T, D, S, K, seed, sep, _ = CASES[name]
        X, phi, spk = planted(T, D, K, seed, sep)
        gamma0, pi0 = init_gamma(noisy_labels(spk, S, seed), S, 5.0)
        _DATA[name] = (X, phi, gamma0, pi0)
    return _DATA[name]


class _Forms(dict):
    """The three runs of one case, each computed when it is first asked for."""

    def __init__(self, name, kw):
        super().__init__()
        self.name, self.kw = name, kw

    def __missing__(self, form):
        X, phi, gamma0, pi0 = case_data(self.name)
        if form == "ld":
            self[form] = vbx_log(X, phi, gamma0, pi0, dtype=np.longdouble, **self.kw)
        elif form == "log":
            self[form] = vbx_log(X, phi, gamma0, pi0, dtype=np.float64, **self.kw)
        elif form == "scaled":
            self[form] = vbx_scaled(X, phi, gamma0, pi0, dtype=np.float64, **self.kw)
        else:
            raise KeyError(form)
        return self[form]


def case_refs(name, epsilon=-np.inf, max_iter=None):
    """{"ld": the longdouble log-domain run, "log": the fp64 log-domain run, "scaled": the fp64 scaled run} of a case, each
    (gamma, pi, elbo, iters), computed once and only when asked for."""
    key = (name, epsilon, max_iter)
    if key not in _REFS:
        _REFS[key] = _Forms(name, dict(OPTS, max_iter=CASES[name][6] if max_iter is None else max_iter, epsilon=epsilon))
    return _REFS[key]


def distances(got, ref):
    """(max |gamma - ref|, max |pi - ref|, max relative |elbo - ref| over the slots the reference ran) as floats."""
    g = float(np.abs(np.asarray(got[0], dtype=np.longdouble) - ref[0]).max())
    p = float(np.abs(np.asarray(got[1], dtype=np.longdouble) - ref[1]).max())
    ran = ~np.isnan(ref[2])
    e = float((np.abs(np.asarray(got[2], dtype=np.longdouble)[ran] - ref[2][ran]) / np.abs(ref[2][ran])).max())
    return g, p, e
