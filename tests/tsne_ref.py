"""numpy float64 restatement of include/xvec_tsne.h -- scikit-learn 1.7's exact t-SNE (_joint_probabilities, _kl_divergence,
_gradient_descent, the schedule of TSNE._tsne) -- and of the PCA the reference plots, with the measures the end-to-end test
compares embeddings by.  A plain module like vad_ref.py: no scikit-learn, no device.  tests/test_tsne.py checks it against
scikit-learn's own functions and against the fixture written from them (tests/golden/g11_tsne.npz)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FLOOR_SUM = float(np.float32(1e-8))        # scikit-learn's `cdef float EPSILON_DBL`
TOLERANCE = float(np.float32(1e-5))        # ... and `cdef float PERPLEXITY_TOLERANCE`
SEARCH_STEPS = 100


def sqdist(x, round_f32=True):
    """euclidean_distances(squared=True) in float64: (-2 x x' + |x_i|^2) + |x_j|^2, clamped at 0, the diagonal 0."""
    x = np.asarray(x, dtype=np.float64)
    xx = np.einsum("ij,ij->i", x, x)
    d = -2.0 * (x @ x.T)
    d += xx[:, None]
    d += xx[None, :]
    np.maximum(d, 0.0, out=d)
    np.fill_diagonal(d, 0.0)
    return d.astype(np.float32).astype(np.float64) if round_f32 else d


def perplexity_search(d2, perplexity):
    """_binary_search_perplexity on every row at once.  Returns (C [n, n] conditional probabilities, betas [n]: the beta C was
    formed with, margin: the smallest distance of any step's | |H - log perplexity| - tolerance | from zero, the steps taken)."""
    d2 = np.asarray(d2, dtype=np.float64)
    n = d2.shape[0]
    off = ~np.eye(n, dtype=bool)
    want = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    used, S = np.ones(n), np.ones(n)
    active = np.ones(n, dtype=bool)
    margin, steps = np.inf, np.zeros(n, dtype=np.int64)
    for _ in range(SEARCH_STEPS):
        rows = np.flatnonzero(active)
        if rows.size == 0:
            break
        e = np.where(off[rows], np.exp(-d2[rows] * beta[rows, None]), 0.0)
        s1 = e.sum(1)
        s1[s1 == 0.0] = FLOOR_SUM
        s2 = (d2[rows] * e).sum(1)
        diff = (np.log(s1) + beta[rows] * (s2 / s1)) - want
        used[rows], S[rows] = beta[rows], s1
        steps[rows] += 1
        margin = min(margin, float(np.abs(np.abs(diff) - TOLERANCE).min()))
        done = np.abs(diff) <= TOLERANCE
        up = diff > 0.0
        b, l, h = beta[rows], lo[rows], hi[rows]
        l = np.where(up, b, l)
        h = np.where(up, h, b)
        nb = np.where(up, np.where(np.isinf(h), b * 2.0, (b + h) / 2.0), np.where(np.isinf(l), b / 2.0, (b + l) / 2.0))
        keep = ~done
        beta[rows[keep]], lo[rows[keep]], hi[rows[keep]] = nb[keep], l[keep], h[keep]
        active[rows[done]] = False
    C = np.where(off, np.exp(-d2 * used[:, None]), 0.0) / S[:, None]
    return C, used, margin, steps


def joint_probabilities(d2, perplexity):
    """Dense symmetric P [n, n]: max((C + C') / max(sum(C + C'), eps), eps) off the diagonal, 0 on it."""
    C = perplexity_search(d2, perplexity)[0]
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def kl_gradient(P, Y, exaggeration=1.0, want_kl=True):
    """(KL, grad [n, 2], Z) of _kl_divergence at degrees_of_freedom = 1 for cP = exaggeration P.  The gradient does NOT floor
    Q at eps (the documented deviation of xvec_tsne.h); the KL value does (None unless `want_kl`)."""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    w = 1.0 / (1.0 + (dx * dx + dy * dy))
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    cP = exaggeration * P
    pw, ww = cP * w, w * w
    attraction = np.stack(((pw * dx).sum(1), (pw * dy).sum(1)), 1)
    repulsion = np.stack(((ww * dx).sum(1), (ww * dy).sum(1)), 1)
    grad = 4.0 * (attraction - repulsion / Z)
    kl = None
    if want_kl:
        iu = np.triu_indices(n, 1)
        kl = 2.0 * float(np.dot(cP[iu], np.log(np.maximum(cP[iu], EPS) / np.maximum(w[iu] / Z, EPS))))
    return kl, grad, Z


def smallest_q(Y):
    """min over pairs of w_ij / Z: the gradient's deviation is void while this stays above eps."""
    Y = np.asarray(Y, dtype=np.float64)
    w = 1.0 / (1.0 + ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    np.fill_diagonal(w, np.inf)
    return float(w.min() / Z)


def steps(P, Y, update, gains, n_steps, exaggeration, momentum, learning_rate, min_gain=0.01):
    """n_steps iterations of _gradient_descent, in place.  Returns (KL of the Y that entered the last iteration, the 2-norm of
    its gradient before the gains)."""
    kl = norm = None
    for k in range(n_steps):
        kl, grad, _ = kl_gradient(P, Y, exaggeration, want_kl=k == n_steps - 1)
        norm = float(np.sqrt((grad ** 2).sum()))
        inc = update * grad < 0.0
        gains[inc] += 0.2
        gains[~inc] *= 0.8
        np.maximum(gains, min_gain, out=gains)
        update[...] = momentum * update - learning_rate * (grad * gains)
        Y += update
    return kl, norm


def _descent(stepper, it, max_iter, patience, min_grad_norm, check, *args):
    """_gradient_descent from iteration `it` over stepper(count, *args, fresh) -> (kl, norm) of the last of `count` iterations;
    `fresh` is set on the first call: scikit-learn starts every descent with a zero update and unit gains.
    Returns (kl, the index of the last iteration run)."""
    kl, best, best_iter, i = np.finfo(float).max, np.finfo(float).max, it, it
    while i < max_iter:
        stop = min(max_iter, (i // check + 1) * check)      # one past the next check iteration, or past the last one
        kl, norm = stepper(stop - i, *args, i == it)
        i = stop
        if stop % check == 0:
            if kl < best:
                best, best_iter = kl, stop - 1
            elif stop - 1 - best_iter > patience:
                break
            if norm <= min_grad_norm:
                break
    return kl, max(i - 1, it)


def schedule(stepper, n, max_iter=1000, early_exaggeration=12.0, learning_rate="auto", n_iter_without_progress=300,
             min_grad_norm=1e-7, exploration=250, check=50):
    """TSNE._tsne's two calls of _gradient_descent (max_iter >= 250, as scikit-learn demands) over
    `stepper(count, exaggeration, momentum, learning_rate, fresh) -> (kl, norm)`.  Returns (kl_divergence_, n_iter_)."""
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    kl, it = _descent(stepper, 0, exploration, exploration, min_grad_norm, check, early_exaggeration, 0.5, lr)
    return _descent(stepper, it + 1, max_iter, n_iter_without_progress, min_grad_norm, check, 1.0, 0.8, lr)


def run(P, Y0, **kw):
    """The whole optimisation from Y0 [n, 2]: (embedding, kl_divergence_, n_iter_)."""
    Y = np.array(Y0, dtype=np.float64)
    update, gains = np.zeros_like(Y), np.ones_like(Y)

    def stepper(count, exaggeration, momentum, lr, fresh):
        if fresh:
            update[...] = 0.0
            gains[...] = 1.0
        return steps(P, Y, update, gains, count, exaggeration, momentum, lr)

    kl, it = schedule(stepper, Y.shape[0], **kw)
    return Y, kl, it


def pca(x, n_components=2, standardize=True):
    """PCA(n_components).fit_transform(StandardScaler().fit_transform(x)) (or of x itself): the eigenvectors of the total
    scatter, largest eigenvalue first, each with its largest-magnitude entry positive (svd_flip(u_based_decision=False)).
    Returns (scores [N, n_components], eigenvalues of the scatter, descending)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    xc = x - mean
    scale = np.ones(x.shape[1])
    if standardize:
        n, var = x.shape[0], (xc ** 2).sum(0) / x.shape[0]
        scale = np.sqrt(var)
        scale[var <= n * EPS * var + (n * mean * EPS) ** 2] = 1.0      # StandardScaler's test for a constant column
    z = xc / scale
    lam, vec = np.linalg.eigh(z.T @ z)
    order = np.argsort(lam)[::-1]
    lam, vec = lam[order], vec[:, order[:n_components]]
    vec = vec * np.sign(vec[np.abs(vec).argmax(0), np.arange(vec.shape[1])])
    return z @ vec, lam


def _ranks(d):
    order = np.argsort(d, axis=1, kind="stable")
    r = np.empty_like(order)
    r[np.arange(d.shape[0])[:, None], order] = np.arange(d.shape[1])[None, :]
    return order, r


def trustworthiness(x, y, k=5):
    """sklearn.manifold.trustworthiness (Euclidean): 1 - 2 / (n k (2n - 3k - 1)) sum_i sum_{j in kNN_y(i)} max(0, r_x(i, j) - k)."""
    dx, dy = sqdist(x, round_f32=False), sqdist(y, round_f32=False)
    np.fill_diagonal(dx, -1.0)
    np.fill_diagonal(dy, -1.0)
    _, rx = _ranks(dx)                     # rank 0 is the point itself
    oy, _ = _ranks(dy)
    n = dx.shape[0]
    nn = oy[:, 1:k + 1]
    t = np.maximum(rx[np.arange(n)[:, None], nn] - k, 0).sum()
    return 1.0 - t * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))


def nn_accuracy(y, labels):
    """Leave-one-out 1-NN label accuracy of an embedding."""
    d = sqdist(y, round_f32=False)
    np.fill_diagonal(d, np.inf)
    labels = np.asarray(labels)
    return float((labels[d.argmin(1)] == labels).mean())


def planted(n_classes=8, per_class=25, dim=64, seed=0, spread=4.0):
    """Planted speakers: `n_classes` Gaussian blobs of `per_class` points (float32) and their labels."""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((n_classes, dim))
    labels = np.repeat(np.arange(n_classes), per_class)
    return (centres[labels] + rng.standard_normal((labels.size, dim))).astype(np.float32), labels
