"""The clustering of include/xvec_diar.h restated in numpy: greedy average linkage (UPGMA) on similarities with the header's
tie and NaN rules, its four-operation update (numpy rounds every elementwise operation on its own) and its canonical labelling.
The matrix is kept in place: `W` the symmetric working copy (NaN on the diagonal and in dead rows and columns), `K` its upper
triangle with everything that cannot be selected at -inf, so that a step is ONE argmax over K (row-major: the first largest
cell is the lowest i, then the lowest j; -0.0 == +0.0).  A plain module like ident_ref.py; the test files import it."""
import numpy as np

NAN, INF = float("nan"), float("inf")


def ahc(S, threshold=INF, max_clusters=0, want=0):
    """(labels int32 [n], n_clusters, merge_i int32 [n], merge_j int32 [n], merge_score float64 [n]) of one recording's block
    S [n, n], of which only the cells with row < column are read.  The merge arrays have the header's n slots: the merges in
    order, then -1, -1, NaN."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    assert S.shape == (n, n) and n >= 1 and not np.isnan(threshold) and max_clusters >= 0 and want >= 0
    iu = np.triu_indices(n, 1)
    W = np.full((n, n), NAN)
    W[iu] = S[iu]
    W.T[iu] = S[iu]
    K = np.full((n, n), -INF)
    K[iu] = np.where(np.isnan(S[iu]), -INF, S[iu])
    size = np.ones(n)
    lab = np.arange(n)
    mi, mj, ms = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, NAN)
    c = n
    for step in range(n - 1):
        flat = int(np.argmax(K))
        i, j = divmod(flat, n)
        best = K[i, j]
        if best == -INF:                       # a masked cell, unless a real -inf cell is what is left
            real = np.flatnonzero(np.triu(W == -INF, 1).ravel())
            if real.size == 0:
                break
            i, j = divmod(int(real[0]), n)
        best = W[i, j]
        if want > 0:
            merge = c > want
        else:
            merge = best >= threshold or (max_clusters > 0 and c > max_clusters)
        if not merge:
            break
        mi[step], mj[step], ms[step] = i, j, best
        with np.errstate(invalid="ignore"):
            row = (size[i] * W[i] + size[j] * W[j]) / (size[i] + size[j])      # two products, a sum, a division
        row[i] = row[j] = NAN                                                  # (dead k: NaN already)
        W[i, :] = row
        W[:, i] = row
        W[j, :] = NAN
        W[:, j] = NAN
        key = np.where(np.isnan(row), -INF, row)
        K[i, i + 1:] = key[i + 1:]
        K[:i, i] = key[:i]
        K[j, :] = -INF
        K[:, j] = -INF
        size[i] += size[j]
        size[j] = 0
        lab[lab == j] = i
        c -= 1
    names = np.flatnonzero(size > 0)           # a cluster's name is its lowest segment: ascending = the canonical order
    rank = np.full(n, -1, np.int32)
    rank[names] = np.arange(names.size, dtype=np.int32)
    return rank[lab], int(names.size), mi, mj, ms


def ahc_batch(S, rec_start, threshold=INF, max_clusters=0, want=None):
    """The same over the diagonal blocks of S: (labels [N], n_clusters [n_rec], merge_i, merge_j, merge_score [N])."""
    out = [ahc(np.asarray(S)[a:b, a:b], threshold, max_clusters, 0 if want is None else int(want[r]))
           for r, (a, b) in enumerate(zip(rec_start[:-1], rec_start[1:]))]
    cat = lambda k: np.concatenate([o[k] for o in out])
    return cat(0), np.array([o[1] for o in out], np.int32), cat(2), cat(3), cat(4)


def planted(n, speakers=4, dim=12, spread=4.0, seed=0):
    """A planted-speaker score matrix [n, n] (symmetric, float64): inner products of `speakers` well separated means plus unit
    noise, speakers in runs of random length as the turns of a conversation are."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((speakers, dim)) * spread
    who = np.zeros(n, dtype=np.int64)
    k, s = 0, 0
    while k < n:
        run = int(rng.integers(1, 9))
        who[k:k + run] = s
        k += run
        s = int(rng.integers(0, speakers))
    x = means[who] + rng.standard_normal((n, dim))
    return x @ x.T / dim, who
