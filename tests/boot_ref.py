"""numpy restatement of the bootstrap (include/xvec_boot.h), the reference of tests/test_bootstrap*.py.  TEST INFRASTRUCTURE
ONLY; a plain module like eer_ref.py.  The Philox is train_dropout_ref's; on top of it the two maps (draw -> group, word ->
Poisson weight, the table from exact rationals), the count tables, the trial weights, the trials in sorted order as the device
leaves them, and one replicate evaluated by the header's definitions in exact integers (int64: every product stays below 2^62
because a replicate of 2^31 or more weighted trials is not evaluated) and float64 without fused operations."""
from fractions import Fraction
from math import factorial

import numpy as np

from train_dropout_ref import philox4x32_10

MAGIC = 0x626F6F74
MAX_GROUPS = 16384
OVERFLOW = 1 << 31
NAN = float("nan")


def _e_inverse(terms=40):
    """1 / e to within 1 / 40! as a rational (alternating series: the error is below the first term left out)."""
    return sum(Fraction((-1) ** k, factorial(k)) for k in range(terms))


def poisson_table():
    """T_i = floor(2^32 P[Poisson(1) <= i]) from exact rationals, up to and including the first that reaches 2^32 - 1."""
    e_inv, out, cdf = _e_inverse(), [], Fraction(0)
    for i in range(64):
        cdf += e_inv / factorial(i)
        out.append(int(cdf * 2 ** 32))            # floor: the value is positive
        assert out[-1] < 2 ** 32
        if out[-1] == 2 ** 32 - 1:
            return out
    raise AssertionError("the table did not end")


POISSON_T = np.array(poisson_table(), dtype=np.uint64)


def words(index, b, side, seed):
    """word index & 3 of philox((index >> 2, b, side, MAGIC), (seed_lo, seed_hi)) for an array of indices."""
    index = np.asarray(index, dtype=np.uint64)
    w = philox4x32_10((index >> np.uint64(2), np.uint64(b), np.uint64(side), np.uint64(MAGIC)),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    sel = (index & np.uint64(3)).astype(np.int64)
    return np.choose(sel, [np.broadcast_to(x, index.shape) for x in w]).astype(np.uint64)


def pick_group(word, n_groups):
    return ((np.asarray(word, dtype=np.uint64) * np.uint64(n_groups)) >> np.uint64(32)).astype(np.int64)


def group_counts(seed, b, side, n_groups):
    """c_s,b [n_groups]: how often each group is picked by the n_groups draws of (seed, b, side)."""
    return np.bincount(pick_group(words(np.arange(n_groups), b, side, seed), n_groups), minlength=n_groups).astype(np.int64)


def poisson_weights(seed, b, t):
    """The Poisson(1) weights of the original trial indices t in replicate b."""
    w = words(t, b, 2, seed)
    return (w[..., None] >= POISSON_T).sum(-1).astype(np.int64)


# ---------------------------------------------------------------- the trials as the device leaves them

def _key_order(scores32):
    """Stable ascending order of float32 scores with -0.0 and +0.0 as one value."""
    return np.argsort(scores32 + np.float32(0.0), kind="stable")


class Sorted:
    """The kept trials in sorted order: score (float32), bit, t (original index), gr / gc (group ids, 0 without the side);
    and the counts of those left out."""

    def __init__(self, scores, rows, cols, target, skip, n_rows, n_cols, row_group, col_group, g_rows, g_cols):
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        n = rows.size
        bad = (rows < 0) | (rows >= n_rows) | (cols < 0) | (cols >= n_cols)
        skip = np.asarray(skip, dtype=bool) & ~bad
        r, c = np.where(bad, 0, rows), np.where(bad, 0, cols)
        gr, gc = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        bad_group = np.zeros(n, dtype=bool)
        if row_group is not None:
            gr = np.asarray(row_group, dtype=np.int64)[r]
            bad_group |= (gr < 0) | (gr >= g_rows)
        if col_group is not None:
            gc = np.asarray(col_group, dtype=np.int64)[c]
            bad_group |= (gc < 0) | (gc >= g_cols)
        bad_group &= ~bad & ~skip
        s = np.asarray(scores, dtype=np.float64)[r, c]
        nan = np.isnan(s) & ~bad & ~skip & ~bad_group
        keep = ~(bad | skip | bad_group | nan)
        self.n_bad_index, self.n_bad_group, self.n_nan = int(bad.sum()), int(bad_group.sum()), int(nan.sum())
        t = np.arange(n)[keep]
        with np.errstate(over="ignore"):
            s32 = s[keep].astype(np.float32)
        order = _key_order(s32)
        self.score, self.t = s32[order] + np.float32(0.0), t[order]
        self.bit = np.asarray(target, dtype=np.int64)[keep][order]
        self.gr, self.gc = gr[keep][order], gc[keep][order]
        self.has_rows, self.has_cols = row_group is not None, col_group is not None
        self.g_rows, self.g_cols = g_rows, g_cols

    @classmethod
    def trials(cls, scores, row_idx, col_idx, is_target, row_group=None, col_group=None, g_rows=0, g_cols=0):
        scores = np.atleast_2d(np.asarray(scores, dtype=np.float64))
        if row_idx is None:
            row_idx, col_idx = np.zeros(len(is_target), dtype=np.int64), np.arange(len(is_target))
        return cls(scores, row_idx, col_idx, np.asarray(is_target) != 0, np.zeros(len(is_target), dtype=bool), scores.shape[0],
                   scores.shape[1], row_group, col_group, g_rows, g_cols)

    @classmethod
    def all_pairs(cls, scores, row_class, col_class, skip_diagonal, row_group=None, col_group=None, g_rows=0, g_cols=0):
        scores = np.asarray(scores, dtype=np.float64)
        rows, cols = np.divmod(np.arange(scores.size), scores.shape[1])
        target = np.asarray(row_class)[rows] == np.asarray(col_class)[cols]
        return cls(scores, rows, cols, target, (rows == cols) & bool(skip_diagonal), scores.shape[0], scores.shape[1], row_group,
                   col_group, g_rows, g_cols)

    def weights(self, seed, b, joint=False):
        """w_b of every kept trial, in sorted order (b = 0: the point estimate, every weight 1)."""
        if b == 0:
            return np.ones(self.t.size, dtype=np.int64)
        if not self.has_rows and not self.has_cols:
            return poisson_weights(seed, b, self.t)
        w = np.ones(self.t.size, dtype=np.int64)
        if self.has_rows:
            w = w * group_counts(seed, b, 0, self.g_rows)[self.gr]
        if self.has_cols:
            w = w * (group_counts(seed, b, 0, self.g_rows) if joint else group_counts(seed, b, 1, self.g_cols))[self.gc]
        return w


# ---------------------------------------------------------------- one replicate

def state(P, A):
    """0 evaluated, 1 degenerate, 2 overflow."""
    if A >= OVERFLOW:
        return 2
    return 1 if P <= 0 or A - P <= 0 else 0


def replicate(srt, w, c_miss=1.0, c_fa=1.0, p_target=0.5):
    """dict of the record's fields (and `state`) of the multiset in which sorted trial k occurs w[k] times."""
    w = np.asarray(w, dtype=np.int64)
    P, A = int((w * srt.bit).sum()), int(w.sum())
    N = A - P
    rec = dict(eer=NAN, eer_threshold=NAN, far=NAN, frr=NAN, min_dcf=NAN, min_dcf_threshold=NAN, n_target=P, n_nontarget=N,
               state=state(P, A))
    if rec["state"]:
        return rec
    tp, ta = np.cumsum(w * srt.bit), np.cumsum(w)
    last = np.r_[srt.score[1:] != srt.score[:-1], True] & (ta > 0)
    k = np.flatnonzero(last)
    tp, nn = tp[k], (ta - tp)[k]
    fa = N - nn
    assert max(P, N) < OVERFLOW                   # |fa P - tp N| < 2^62: int64 is exact
    e = int(np.argmin(np.abs(fa * P - tp * N)))   # the first minimum
    frr, far = tp / P, fa / N                     # float64 quotients of exact integers
    c_det = c_miss * frr * p_target + c_fa * far * (1.0 - p_target)
    d = int(np.argmin(c_det))
    rec.update(eer=(far[e] + frr[e]) / 2.0, eer_threshold=float(srt.score[k[e]]), far=float(far[e]), frr=float(frr[e]),
               min_dcf=float(c_det[d]), min_dcf_threshold=float(srt.score[k[d]]))
    return rec


def bootstrap(srt, n_boot, seed, joint=False, c_miss=1.0, c_fa=1.0, p_target=0.5, replicates=None):
    """(records 0 .. n_boot as dicts, summary dict); `replicates`: evaluate only these b (the others are None)."""
    want = range(n_boot + 1) if replicates is None else replicates
    recs = [None] * (n_boot + 1)
    for b in want:
        recs[b] = replicate(srt, srt.weights(seed, b, joint), c_miss, c_fa, p_target)
    done = [r for b, r in enumerate(recs) if r is not None and b >= 1]
    summary = dict(n_nan=srt.n_nan, n_bad_index=srt.n_bad_index, n_bad_group=srt.n_bad_group,
                   n_degenerate=sum(r["state"] == 1 for r in done), n_overflow=sum(r["state"] == 2 for r in done))
    return recs, summary


def expanded(srt, w):
    """(pos, neg): the literally expanded score lists, every trial repeated w times (for eer_ref.naive / by_sort)."""
    s = np.repeat(srt.score.astype(np.float64), w)
    bit = np.repeat(srt.bit, w)
    return s[bit == 1], s[bit == 0]


def percentile_ranks(m, level):
    """The header rule of bootstrap.percentile_ranks in exact rationals."""
    alpha = (1 - Fraction(level).limit_denominator(10 ** 6)) / 2
    k_lo = max(1, int((m + 1) * alpha))
    return k_lo, m + 1 - k_lo
