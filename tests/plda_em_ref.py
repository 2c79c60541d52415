"""Literal numpy/scipy restatement of speechbrain 0.5.12's PLDA training, default path (PLDA_LDA.PLDA.plda with
whiten=False): per-iteration whitening by eigh(Sigma), a per-class E-step with one inv(n A + I) per distinct class size,
the accumulators _R, _C, _A, the M-step and the minimum-divergence step with scipy's upper Cholesky factor.

UNPINNED against speechbrain itself: the package is not installed and the reference holds no test vectors; this is a
reading of its published algorithm, used to check xvector_amd.plda (which computes the same thing rewritten).  Also here:
a generator of labelled vectors from a known two-covariance model."""
import numpy as np
from scipy import linalg


def class_stats(x, labels, scaling_factor=1.0):
    """mean [D], sigma_obs [D, D] (biased), class names (sorted), counts [C] and class sums [C, D] (both scaled,
    the sums NOT centred), numpy float64."""
    x = np.asarray(x, dtype=np.float64)
    classes, inv = np.unique(np.asarray(labels), return_inverse=True)
    inv = inv.reshape(-1)
    mean = x.mean(0)
    xc = x - mean
    sigma_obs = xc.T @ xc / x.shape[0]
    sums = np.zeros((classes.shape[0], x.shape[1]))
    np.add.at(sums, inv, x)
    counts = np.bincount(inv, minlength=classes.shape[0]).astype(np.float64)
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
