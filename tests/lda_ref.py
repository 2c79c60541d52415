"""The arithmetic of include/xvec_lda.h and xvector_amd.lda restated in numpy (float64, or `dtype=np.longdouble` to show how far
float64 itself is from the exact result): the LDA statistics, the speechbrain-shaped route to the LDA matrix
(`eig(inv(Sw) @ Sb)`), whitening, the norm clip, and the error bounds the device tests hold the kernels to.  A plain module
like plda_em_ref.py; the test files import it.

Bounds.  A value computed as a sum of `terms` products a_k b_k in float64 with fused multiply-adds, from operands that each
carry up to two roundings of their own (a subtraction, a weight), lies within
    (terms + 4) 2^-53 sum_k |a_k| |b_k|
of the exact value to first order -- the form of the PLDA and score edge tests.  Each stage is held to it on the operands the
stage is GIVEN: the scatter matrices are the kernel's formula in np.longdouble on x and on the class means / mean the device
itself returned (those are held to their own bound against x).  The reason is arithmetic, not convenience: s_between is a
product of differences of float64 means, and no float64 mean is closer to the exact one than half an ulp OF THE MEAN, which
under a common offset is far more than 2^-53 of the difference.  s_within does not suffer from this: a perturbation d of a class
mean changes the class's term by exactly d d' (the centred rows sum to zero), second order.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
NORM_CLIP = 1e-8


def make_case(n, dim, n_classes, offset=0.0, seed=1234):
    """The synthetic generator of the LDA tests: class means scaled 3 * 0.5^k along random orthogonal directions, noise 0.3
    (growing to 0.6 over the dimensions), every class present.  (x [n, dim] float64, labels [n])."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_classes, n)
    lab[:n_classes] = np.arange(n_classes)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    cm = np.zeros((n_classes, dim))
    for c in range(n_classes):
        cm[c] = rng.standard_normal(dim)
    cm = (cm * (3.0 * 0.5 ** np.arange(dim))) @ q.T
    x = cm[lab] + 0.3 * rng.standard_normal((n, dim)) * (1 + np.arange(dim) / dim) + offset
    return x, lab


def lda_stats(x, labels, dtype=np.float64, class_means=None, mean=None, rows=None):
    """(mean [D], class_means [C, D], s_within [D, D], s_between [D, D], classes) by the definitions of include/xvec_lda.h.
    `class_means` / `mean` given: the scatter matrices are formed around THOSE (the operands the device kernels are given).
    `rows` given: only those rows of the two matrices ([len(rows), D])."""
    x = np.asarray(x, dtype=dtype)
    classes = np.unique(labels)
    dim = x.shape[1]
    mu = x.sum(0) / dtype(x.shape[0])
    cm = np.zeros((len(classes), dim), dtype=dtype)
    sel = slice(None) if rows is None else rows
    sw = np.zeros((dim, dim), dtype=dtype)[sel]
    for k, c in enumerate(classes):
        xc = x[np.asarray(labels) == c]
        cm[k] = xc.sum(0) / dtype(xc.shape[0])
        t = xc - (cm[k] if class_means is None else np.asarray(class_means[k], dtype=dtype))
        sw += (t[:, sel] / dtype(xc.shape[0])).T @ t
    a = (cm if class_means is None else np.asarray(class_means, dtype=dtype)) - (mu if mean is None else np.asarray(mean, dtype=dtype))
    return mu, cm, sw, a[:, sel].T @ a, classes


def lda_stats_bounds(x, labels, class_means, mean, rows=None):
    """Element-wise bounds (float64 arrays) for (mean, class_means, s_within, s_between) of the device, in the form of the
    module docstring: mean and class_means against x, the scatter matrices against lda_stats(..., class_means, mean, rows)."""
    x = np.asarray(x, dtype=LD)
    classes = np.unique(labels)
    n, dim = x.shape
    b_mean = (n + 4) * U * np.abs(x).sum(0) / n
    b_cm = np.zeros((len(classes), dim), dtype=LD)
    sel = slice(None) if rows is None else rows
    s_abs = np.zeros((dim, dim), dtype=LD)[sel]
    for k, c in enumerate(classes):
        xc = x[np.asarray(labels) == c]
        b_cm[k] = (xc.shape[0] + 4) * U * np.abs(xc).sum(0) / xc.shape[0]
        t = np.abs(xc - np.asarray(class_means[k], dtype=LD))
        s_abs += (t[:, sel] / xc.shape[0]).T @ t
    a = np.abs(np.asarray(class_means, dtype=LD) - np.asarray(mean, dtype=LD))
    f = lambda v: np.asarray(v, dtype=np.float64)
    return f(b_mean), f(b_cm), f((n + 4) * U * s_abs), f((len(classes) + 4) * U * (a[:, sel].T @ a))


def sign_rule(L):
    """Columns of unit 2-norm with the largest-magnitude component positive."""
    L = np.asarray(L)
    L = L / np.linalg.norm(L, axis=0)
    return L * np.sign(L[np.abs(L).argmax(0), np.arange(L.shape[1])])


def lda_matrix_eig(sw, sb, rank):
    """speechbrain's route: eig(inv(Sw) @ Sb), the real parts sorted descending, the top `rank` eigenvectors -- then the
    sign rule.  Returns (matrix [D, rank] real, largest imaginary part met)."""
    from scipy import linalg
    ev, evec = linalg.eig(np.linalg.inv(sw) @ sb)
    idx = np.real(ev).argsort()[-rank:][::-1]
    L = evec[:, idx]
    return sign_rule(np.real(L)), float(np.abs(np.imag(L)).max())


def whitening_matrix(sigma):
    """speechbrain's whiten_stat1: eigh, eigenvalues descending, V diag(1 / sqrt(lam)); 1-D sigma: diag(1 / sqrt(sigma))."""
    from scipy import linalg
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim == 1:
        return np.diag(1.0 / np.sqrt(sigma))
    ev, evec = linalg.eigh(sigma)
    ind = ev.argsort()[::-1]
    return evec[:, ind] @ np.diag(1.0 / np.sqrt(ev[ind]))


def norm_rows(y):
    """speechbrain's norm_stat1: every row divided by clip(its 2-norm, 1e-8)."""
    y = np.asarray(y)
    nrm = np.sqrt((y * y).sum(1))
    return y / np.maximum(nrm, y.dtype.type(NORM_CLIP))[:, None]


def transform(x, mean=None, w=None, normalize=False, dtype=np.float64):
    """(x - mean) w, rows normalised if asked: the definition of xvec_embed_transform."""
    y = np.asarray(x, dtype=dtype)
    if mean is not None:
        y = y - np.asarray(mean, dtype=dtype)
    if w is not None:
        y = y @ np.asarray(w, dtype=dtype)
    return norm_rows(y) if normalize else y


def transform_bound(x, mean, w, normalize):
    """Element-wise bound (np.longdouble: the one-rounding bound of the bare centring is met exactly at ties, so it must not be
    rounded itself) for xvec_embed_transform against transform(..., dtype=np.longdouble).
    Product: (dim + 4) 2^-53 (|x - mean| |w|) (w None: one rounding of the subtraction, 2^-53 |x - mean| -- exact zero where
    there is no mean).  Normalised: with b the product's bound, y the exact product and nrm = max(||y||, 1e-8), the computed
    sum of squares is off by at most 2 sum |y_j| b_j (its operands) + (rank + 2) 2^-53 ||y||^2 (its own roundings), so the
    norm by a relative e = sum |y_j| b_j / ||y||^2 + (rank / 2 + 3) 2^-53 (square root and clip included), and the quotient by b / nrm + |y| / nrm (e + 2^-53)."""
    xl = np.asarray(x, dtype=LD)
    xc = np.abs(xl - np.asarray(mean, dtype=LD)) if mean is not None else np.abs(xl)
    if w is not None:
        b = (xl.shape[1] + 4) * U * (xc @ np.abs(np.asarray(w, dtype=LD)))
    else:
        b = U * xc if mean is not None else np.zeros_like(xc)
    if not normalize:
        return b
    y = transform(x, mean, w, False, dtype=LD)
    ay = np.abs(y)
    n2 = (y * y).sum(1)
    nrm = np.maximum(np.sqrt(n2), LD(NORM_CLIP))
    safe = np.where(n2 > 0, n2, LD(1))
    e = (ay * b).sum(1) / safe + (y.shape[1] / 2 + 3) * U
    return b / nrm[:, None] + ay / nrm[:, None] * (e + U)[:, None]
