"""Literal numpy/scipy restatement of speechbrain 0.5.12's PLDA training, default path (PLDA_LDA.PLDA.plda with
whiten=False): per-iteration whitening by eigh(Sigma), a per-class E-step with one inv(n A + I) per distinct class size,
the accumulators _R, _C, _A, the M-step and the minimum-divergence step with scipy's upper Cholesky factor.

UNPINNED against speechbrain itself: the package is not installed and the reference holds no test vectors; this is a
reading of its published algorithm, used to check xvector_amd.plda (which computes the same thing rewritten).  Also here:
a generator of labelled vectors from a known two-covariance model."""
import numpy as np
from scipy import linalg


def class_stats(x, labels, scaling_factor=1.0, dtype=np.float64):
    """mean [D], sigma_obs [D, D] (biased), class names (sorted), counts [C] and class sums [C, D] (both scaled,
    the sums NOT centred), numpy float64 (or `dtype`: np.longdouble shows how far float64 itself is from the exact result)."""
    x = np.asarray(x, dtype=dtype)
    classes, inv = np.unique(np.asarray(labels), return_inverse=True)
    inv = inv.reshape(-1)
    mean = x.mean(0)
    xc = x - mean
    sigma_obs = xc.T @ xc / x.shape[0]
    sums = np.zeros((classes.shape[0], x.shape[1]), dtype=dtype)
    np.add.at(sums, inv, x)
    counts = np.bincount(inv, minlength=classes.shape[0]).astype(dtype)
    return mean, sigma_obs, classes, counts * scaling_factor, sums * scaling_factor


def plda_em(x, labels, rank_f, nb_iter=10, scaling_factor=1.0):
    """(mean, F, Sigma) of speechbrain's PLDA.plda on stat1 = x, modelset = labels."""
    mean, sigma_obs, classes, counts, sums = class_stats(x, labels, scaling_factor)
    class_nb, vect_size = sums.shape
    evals, evecs = linalg.eigh(sigma_obs)
    idx = np.argsort(evals)[::-1]
    F = evecs.real[:, idx[:rank_f]]
    Sigma = sigma_obs.copy()
    shifted = sums - counts[:, None] * mean            # center_stat1: stat1 - stat0 * mean
    for _ in range(nb_iter):
        # whiten_stat1(mean, Sigma)
        ev, V = linalg.eigh(Sigma)
        ind = ev.real.argsort()[::-1]
        ev, V = ev.real[ind], V.real[:, ind]
        sqr_inv_sigma = V @ np.diag(1.0 / np.sqrt(ev))
        stat1 = shifted @ sqr_inv_sigma
        F = sqr_inv_sigma.T @ F
        # fa_model_loop
        A = F.T @ F
        inv_lambda_unique = {n: linalg.inv(n * A + np.eye(A.shape[0])) for n in np.unique(counts)}
        e_h = np.zeros((class_nb, rank_f))
        e_hh = np.zeros((class_nb, rank_f, rank_f))
        for c in range(class_nb):
            inv_lambda = inv_lambda_unique[counts[c]]
            aux = F.T @ stat1[c]
            e_h[c] = aux @ inv_lambda
            e_hh[c] = inv_lambda + np.outer(e_h[c], e_h[c])
        _R = e_hh.sum(0) / class_nb
        _C = e_h.T @ stat1 @ linalg.inv(sqr_inv_sigma)
        _A = np.einsum("ijk,i->jk", e_hh, counts)
        F = linalg.solve(_A, _C).T
        Sigma = sigma_obs - F @ _C / counts.sum()
        F = F @ linalg.cholesky(_R)
    return mean, F, Sigma


def em_products_bound(sums_centred, counts, pq, lam):
    """Element-wise error bounds (E_hh, E_nhh, E_hs) of the E-step products H'H, H' diag(n) H, H'S computed in float64 in
    any summation order, with S = sums_centred [C, D], pq [D, R], H = (S pq) / (n lam + 1).  Derived, u = 2^-53:
       a K-term product   |fl(A B') - A B'| <= (K + 8) u (|A| |B|'), whatever the order of the sum (the 8 is room for the
                          second-order terms and for the roundings around the sum)
       Y = S pq           E_Y = (D + 8) u (|S| |pq|)
       H = Y / (n lam+1)  the denominator is positive and formed as one fused multiply-add or as a product and a sum, then the
                          division: E_H = E_Y / (n lam + 1) + 2 u |H| (an unfused n lam adds u |H| <= u |S||pq| / (n lam + 1),
                          inside the 8 u of E_Y)
       n H                one more rounding: E_nH = n E_H + u |n H|
       products of H      K = C, on operands that are themselves off by E_H: with Hb = |H| + E_H >= |computed H| and
                          nHb = |n H| + E_nH
                          E_hh  = (C + 8) u Hb' Hb  + Hb' E_H + E_H' Hb
                          E_nhh = (C + 8) u Hb' nHb + E_H' nHb + Hb' E_nH
                          E_hs  = (C + 8) u Hb' |S| + E_H' |S|           (S is an input: exact)
    The bound terms themselves are formed in float64: they are sums of non-negative numbers, good to 1e-15 of themselves."""
    S = np.abs(np.asarray(sums_centred, dtype=np.float64))
    n = np.asarray(counts, dtype=np.float64)[:, None]
    P = np.asarray(pq, dtype=np.float64)
    u = 2.0 ** -53
    C, D = S.shape
    den = n * np.asarray(lam, dtype=np.float64)[None, :] + 1.0
    H = np.abs(np.asarray(sums_centred, dtype=np.float64) @ P) / den
    E_H = (D + 8) * u * (S @ np.abs(P)) / den + 2 * u * H
    E_nH = n * E_H + u * n * H
    Hb, nHb = H + E_H, n * H + E_nH
    k = (C + 8) * u
    return (k * Hb.T @ Hb + Hb.T @ E_H + E_H.T @ Hb, k * Hb.T @ nHb + E_H.T @ nHb + Hb.T @ E_nH,
            k * Hb.T @ S + E_H.T @ S)


def make_data(n_classes, dim, rank, sizes=(1, 40), seed=0, offset=3.0, between=1.0):
    """x = mu + F_true y_s + eps, eps ~ N(0, Sigma_true), y_s ~ N(0, I): uneven class sizes in [sizes[0], sizes[1]],
    rows shuffled so that labels are not grouped.  Returns x [N, dim], labels [N] (int), (mu, F_true, Sigma_true)."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, offset, dim)
    F_true = rng.normal(0, between, (dim, rank))
    B = rng.normal(0, 1, (dim, dim)) / np.sqrt(dim)
    Sigma_true = B @ B.T + 0.5 * np.eye(dim)
    L = np.linalg.cholesky(Sigma_true)
    n_per = rng.integers(sizes[0], sizes[1] + 1, n_classes)
    labels = np.repeat(np.arange(n_classes), n_per)
    y = rng.normal(0, 1, (n_classes, rank))
    x = mu + (y @ F_true.T)[labels] + rng.normal(0, 1, (labels.shape[0], dim)) @ L.T
    perm = rng.permutation(labels.shape[0])
    return x[perm], labels[perm], (mu, F_true, Sigma_true)


def rel(a, b):
    """Frobenius-relative difference."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))
