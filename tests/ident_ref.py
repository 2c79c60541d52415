"""The definitions of include/xvec_ident.h restated in numpy from the published code of speechbrain 0.5.12
(processing/PLDA_LDA.py): StatObject_SB.mean_stat_per_model (the boolean-mask mean per model), the open-set loop of
fast_PLDA_scoring's `p_known != 0` branch exactly as written there, and top-k by a stable argsort; besides them the open-set
scores in np.longdouble, shifted by the column maximum so that they stay finite at scores of +-900.  Parity with speechbrain
itself is unpinned (the package is not installed in the build image, as tests/test_scoring.py says of the scorer).  A plain
module like snorm_ref.py and lda_ref.py; the test files import it."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def model_means(x, names, dtype=np.float64):
    """(unique names, [M, D] means): `sts_per_model.modelset = numpy.unique(self.modelset)`, then per model
    `numpy.mean(self.stat1[self.modelset == model, :], axis=0)`; with dtype=LD the sums run in longdouble."""
    names = np.asarray(names)
    x = np.asarray(x)
    models = np.unique(names)
    out = np.zeros((models.shape[0], x.shape[1]), dtype=dtype)
    for idx, model in enumerate(models):
        out[idx] = np.mean(x[names == model, :].astype(dtype), axis=0)
    return models, out


def model_mean_bound(x, names):
    """[M, D] per-element bound of a model's mean, any summation order: n_c - 1 roundings on the way to the sum, one for the
    division, one spare: (n_c + 2) u sum |x| / n_c."""
    names = np.asarray(names)
    x = np.abs(np.asarray(x, dtype=np.float64))
    models = np.unique(names)
    out = np.zeros((models.shape[0], x.shape[1]))
    for idx, model in enumerate(models):
        rows = x[names == model]
        out[idx] = (rows.shape[0] + 2) * U * rows.sum(axis=0) / rows.shape[0]
    return out


def open_set_loop(scoremat, p_known):
    """The package's loop, fp64, as written:
        N = scoremat.shape[0]; open_set_scores = numpy.empty(scoremat.shape); tmp = numpy.exp(scoremat)
        for ii in range(N):
            open_set_scores[ii, :] = scoremat[ii, :] - numpy.log(
                p_known * tmp[~(numpy.arange(N) == ii)].sum(axis=0) / (N - 1) + (1 - p_known))
    It overflows beyond scores of about 709: for benign scores only."""
    scoremat = np.asarray(scoremat, dtype=np.float64)
    N = scoremat.shape[0]
    open_set_scores = np.empty(scoremat.shape)
    tmp = np.exp(scoremat)
    for ii in range(N):
        open_set_scores[ii, :] = scoremat[ii, :] - np.log(
            p_known * tmp[~(np.arange(N) == ii)].sum(axis=0) / (N - 1) + (1 - p_known))
    return open_set_scores


def open_set_longdouble(scoremat, p_known):
    """(out, L, W) in np.longdouble: out = S - L with L[i, j] = log(p sum_{k != i} exp S[k, j] / (N - 1) + (1 - p)) formed as
    m + log(p sum_{k != i} exp(S[k, j] - m) / (N - 1) + (1 - p) exp(-m)) for m = the column maximum > 0 and as
    log(exp(m) p sum / (N - 1) + (1 - p)) otherwise, and W[j] = max_k |S[k, j] - m|.  The sum over k != i is a direct sum of
    its N - 1 positive terms (the rows before i, left to right, plus the rows after i, right to left: no term is ever
    subtracted).  Columns with a NaN cell are NaN; -inf cells add 0."""
    s = np.asarray(scoremat, dtype=np.float64).astype(LD)
    N = s.shape[0]
    p = LD(p_known)
    with np.errstate(all="ignore"):
        m = s.max(axis=0)
        fin = np.where(np.isfinite(m), m, LD(0))
        e = np.exp(s - fin[None, :])                               # exp(-inf) = 0
        zero = np.zeros((1, s.shape[1]), dtype=LD)
        before = np.concatenate([zero, np.cumsum(e, axis=0)[:-1]], axis=0)
        after = np.concatenate([np.cumsum(e[::-1], axis=0)[::-1][1:], zero], axis=0)
        others = before + after
        up = fin > 0
        rest = np.where(up, (LD(1) - p) * np.exp(-fin), LD(1) - p)
        scale = np.where(up, LD(1), np.exp(fin))
        L = np.where(up, fin, LD(0))[None, :] + np.log(scale[None, :] * (p * others / LD(N - 1)) + rest[None, :])
        diff = np.abs(s - fin[None, :])
        W = np.where(np.isfinite(diff), diff, LD(0)).max(axis=0)
        out = s - L
    return out, L, W.astype(np.float64)


def open_set_bound(scoremat, out, L, W):
    """2^-53 [(N + 8 + W_j) + 2 |L_ij| + |out_ij| + |S_ij|] per cell: the relative error of a sum of N positive terms in any
    order (N u), |x| u for the rounded argument of every exp (|S - m1| <= W_j), the ulps of exp, of log and of the operations
    between them (the 8), the roundings of L = m1 + log(.) (2 |L| u: the sum and the argument's scale), the final subtraction
    (|out| u) and the rounding of S - m1 itself at the scale of S (|S| u)."""
    s = np.abs(np.asarray(scoremat, dtype=np.float64))
    N = s.shape[0]
    with np.errstate(all="ignore"):
        return U * ((N + 8 + W[None, :]) + 2 * np.abs(L.astype(np.float64)) + np.abs(out.astype(np.float64)) + s)


def total_minus_own(scoremat, p_known):
    """The shortcut the library must NOT take: column total minus the row's own term, fp64, shifted by the column maximum."""
    s = np.asarray(scoremat, dtype=np.float64)
    N = s.shape[0]
    m = s.max(axis=0)
    e = np.exp(s - m[None, :])
    others = e.sum(axis=0)[None, :] - e
    with np.errstate(all="ignore"):
        return s - (m[None, :] + np.log(p_known * others / (N - 1) + (1 - p_known) * np.exp(-m)[None, :]))


def open_set_algorithm(scoremat, p_known, slice_rows=32, block_rows=128):
    """The library's algorithm (include/xvec_ident.h) in numpy fp64, column by column: (m1, i1, R) per slice, merged with
    rescaling in slice order inside a block and in block order across blocks, then the branch rule.  For the CPU check of the
    algorithm against the longdouble form."""
    s = np.asarray(scoremat, dtype=np.float64)
    N, T = s.shape
    ninf = -np.inf
    out = np.empty_like(s)

    def ex(x, m):
        return 0.0 if x == ninf else float(np.exp(np.float64(x - m)))

    def part(col, r0, r1):
        if r0 >= r1:
            return (ninf, 0.0, -1)
        seg = col[r0:r1]
        if np.isnan(seg).any():
            return (np.nan, np.nan, r0)
        at = int(np.argmax(seg))
        m, R = float(seg[at]), 0.0
        for k in range(r1 - r0):
            if k != at:
                R += ex(seg[k], m)
        return (m, R, r0 + at)

    def merge(a, b):
        if np.isnan(a[0]) or np.isnan(b[0]):
            return (np.nan, np.nan, a[2] if np.isnan(a[0]) else b[2])
        if a[2] < 0 or b[0] > a[0]:
            return (b[0], ((a[1] + 1.0) * ex(a[0], b[0]) if a[2] >= 0 else 0.0) + b[1], b[2])
        return (a[0], a[1] + ((b[1] + 1.0) * ex(b[0], a[0]) if b[2] >= 0 else 0.0), a[2])

    p = float(p_known)
    with np.errstate(all="ignore"):
        for j in range(T):
            col = s[:, j]
            total = None
            for b0 in range(0, N, block_rows):
                blk = None
                for r0 in range(b0, b0 + block_rows, slice_rows):
                    q = part(col, r0, min(r0 + slice_rows, N))
                    blk = q if blk is None else merge(blk, q)
                total = blk if total is None else merge(total, blk)
            m1, R, i1 = total
            shifted = m1 > 0.0 or p == 1.0
            rest = 1.0 - p
            c = (0.0 if p == 1.0 else rest * np.exp(-m1)) if shifted else np.exp(m1)
            for i in range(N):
                A = R if i == i1 else 1.0 + (R - ex(col[i], m1))
                q = (p * A) / float(N - 1)
                L = m1 + np.log(q + c) if shifted else np.log(c * q + rest)
                out[i, j] = col[i] - L
    return out


def topk(scoremat, k):
    """(idx [k, T] int32, val [k, T] float64) by a stable argsort per column: larger score first, equal scores (-0.0 == +0.0)
    by lower row; NaN cells are never taken; places that cannot be filled hold -1 and NaN."""
    s = np.asarray(scoremat, dtype=np.float64)
    N, T = s.shape
    idx = np.full((k, T), -1, dtype=np.int32)
    val = np.full((k, T), np.nan)
    for j in range(T):
        col = s[:, j]
        rows = np.nonzero(~np.isnan(col))[0]
        key = -(col[rows] + 0.0)                     # -0.0 + 0.0 = +0.0: the two zeros tie
        best = rows[np.argsort(key, kind="stable")][:k]
        idx[:best.size, j] = best
        val[:best.size, j] = col[best]
    return idx, val


def decide(idx, val, threshold):
    """[T] int32: the best model if its score >= threshold, else -1."""
    with np.errstate(invalid="ignore"):
        return np.where((idx[0] >= 0) & (val[0] >= threshold), idx[0], -1).astype(np.int32)
