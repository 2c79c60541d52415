"""The numpy oracle of score analysis (include/xvec_analyze.h): which trials count, the moments in np.longdouble, the bins by
numpy's floor and rint, the hardest lists by a stable lexsort on (key, t), the Gaussian KDE of binned values, and the numbers
the reference's extra/compare_speaker_results.py prints.  A plain module like boot_ref.py; the test files import it."""
import numpy as np

RECORD = np.dtype([("score", "<f8"), ("row", "<i4"), ("col", "<i4"), ("t", "<i8")])
FLOOR, RINT = 0, 1


class Usable:
    """The trials that take part, in trial order: s, target (bool), t, row, col; and what was left out."""

    def __init__(self, s, target, t, row, col, n_nan, n_bad):
        self.s, self.target, self.t, self.row, self.col = s, target.astype(bool), t, row, col
        self.n_nan, self.n_bad = int(n_nan), int(n_bad)

    def of(self, which):
        m = np.ones(len(self.s), bool) if which == 2 else (self.target == bool(which))
        return self.s[m], self.t[m], self.row[m], self.col[m]


def usable_trials(scores, rows, cols, tgt):
    scores = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    n = len(tgt)
    t = np.arange(n, dtype=np.int64)
    rows = np.zeros(n, np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = t.copy() if cols is None else np.asarray(cols, dtype=np.int64)
    ok = (rows >= 0) & (rows < scores.shape[0]) & (cols >= 0) & (cols < scores.shape[1])
    s = np.full(n, 0.0)
    s[ok] = scores[rows[ok], cols[ok]]
    nan = ok & np.isnan(s)
    keep = ok & ~nan
    return Usable(s[keep], np.asarray(tgt)[keep] != 0, t[keep], rows[keep], cols[keep], nan.sum(), (~ok).sum())


def usable_all_pairs(scores, row_class, col_class, skip_diagonal=True, upper_only=False):
    scores = np.asarray(scores, dtype=np.float64)
    n_rows, n_cols = scores.shape
    row, col = np.divmod(np.arange(n_rows * n_cols, dtype=np.int64), n_cols)
    part = np.ones(n_rows * n_cols, bool)
    if skip_diagonal:
        part &= row != col
    if upper_only:
        part &= row < col
    s = scores.reshape(-1)
    nan = part & np.isnan(s)
    keep = part & ~nan
    target = np.asarray(row_class)[row] == np.asarray(col_class)[col]
    t = np.arange(n_rows * n_cols, dtype=np.int64)
    return Usable(s[keep], target[keep], t[keep], row[keep], col[keep], nan.sum(), 0)


# ---------------------------------------------------------------- moments

def moments(s, t):
    """n, min, max with the lowest t that attains each, mean and population variance, summed in np.longdouble."""
    n = len(s)
    if n == 0:
        return dict(n=0, min=np.nan, max=np.nan, t_min=-1, t_max=-1, mean=np.nan, var=np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        x = s.astype(np.longdouble)
        mean = x.sum() / n
        var = ((x - mean) ** 2).sum() / n
    return dict(n=n, min=float(s.min()), max=float(s.max()), t_min=int(t[np.argmin(s)]), t_max=int(t[np.argmax(s)]), mean=mean,
                var=var)


def summary(u: Usable):
    return [moments(*u.of(c)[:2]) for c in (0, 1, 2)]


# ---------------------------------------------------------------- bins

def slots(s, width, first, n_bins, rounding):
    """Slot of every score among n_bins + 2: 0 underflow, b + 1 bin b, n_bins + 1 overflow."""
    with np.errstate(over="ignore"):
        q = np.asarray(s, dtype=np.float64) / np.float64(width)
    r = np.rint(q) if rounding == RINT else np.floor(q)
    out = np.zeros(len(r), dtype=np.int64)
    out[r > first + n_bins - 1] = n_bins + 1
    inside = (r >= first) & (r <= first + n_bins - 1)
    out[inside] = r[inside].astype(np.int64) - first + 1
    return out


def histogram(u: Usable, width, first, n_bins, rounding):
    """int64 [2][n_bins + 2]"""
    return np.stack([np.bincount(slots(u.of(c)[0], width, first, n_bins, rounding), minlength=n_bins + 2) for c in (0, 1)])


# ---------------------------------------------------------------- hardest

def key_of(s):
    """The order-preserving 64-bit key of csrc/snorm_keys.h: key(a) < key(b) iff a < b; the two zeros share one."""
    u = np.asarray(s, dtype=np.float64).copy()
    u[u == 0.0] = 0.0
    b = u.view(np.uint64)
    sign = np.uint64(1) << np.uint64(63)
    return np.where(b & sign != 0, ~b, b | sign)


def hardest(u: Usable, k):
    """(the k highest non-target, the k lowest target) as RECORD arrays, the hardest first, ties to the lower t."""
    out = []
    for c in (0, 1):
        s, t, row, col = u.of(c)
        key = key_of(s)
        if c == 0:
            key = ~key                       # descending value
        order = np.lexsort((t, key))[:k]     # key first, then t; stable
        rec = np.zeros(len(order), dtype=RECORD)
        rec["score"], rec["row"], rec["col"], rec["t"] = s[order], row[order], col[order], t[order]
        out.append(rec)
    return out


def reference_false_positives(neg_scores, k):
    """The loop of extra/compare_speaker_results.py:105-115 on a matrix that is 0 off the non-target cells: the maximum, every
    cell that attains it, those cells set to 0 -- k times.  Returns [(score, rows, cols)]."""
    m = np.array(neg_scores, dtype=np.float64)
    hits = []
    for _ in range(k):
        top = np.max(m)
        index = np.where(m == top)
        hits.append((top, index[0].copy(), index[1].copy()))
        for i, j in zip(index[0], index[1]):
            m[i, j] = 0
    return hits


# ---------------------------------------------------------------- density

def density(values, counts, gridsize=100, cut=3, bw="scott"):
    """Gaussian KDE of the values repeated `counts` times: (grid, density); h = n^(-1/5) std(ddof=1), or `bw` itself."""
    values, counts = np.asarray(values, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    keep = counts > 0
    values, counts = values[keep], counts[keep]
    n = counts.sum()
    mean = (values * counts).sum() / n
    std = np.sqrt((counts * (values - mean) ** 2).sum() / (n - 1))
    h = n ** (-0.2) * std if bw == "scott" else float(bw)
    grid = np.linspace(values.min() - cut * h, values.max() + cut * h, gridsize)
    z = (grid[:, None] - values[None, :]) / h
    dens = (np.exp(-0.5 * z * z) * counts[None, :]).sum(axis=1) / (n * h * np.sqrt(2.0 * np.pi))
    return grid, dens


# ---------------------------------------------------------------- the reference's lists and prints

def speaker_number(name):
    return int(str(name).split("/")[0][2:])


def confusable_pairs(records, row_names, col_names):
    """pairs (unordered speaker pairs in order of first appearance), num_pairs (the pair number of every hit, 1-based) and
    performance (the scores), as extra/compare_speaker_results.py:120-128 builds them for the hits it prints."""
    pairs, num_pairs, performance = [], [], []
    for r in records:
        a, b = sorted((speaker_number(row_names[r["row"]]), speaker_number(col_names[r["col"]])))
        if (a, b) not in pairs:
            pairs.append((a, b))
        num_pairs.append(pairs.index((a, b)) + 1)
        performance.append(float(r["score"]))
    return pairs, num_pairs, performance


def compare_speaker_results(scoremat, modelset, segset, k=100):
    """Every number the reference script prints: the target mask from the id prefixes, the diagonal included."""
    scoremat = np.asarray(scoremat, dtype=np.float64)
    spk = lambda names: np.array([str(n).split(".")[0].split("/")[0] for n in names])
    pos = spk(modelset)[:, None] == spk(segset)[None, :]
    out = {}
    for name, x in (("all", scoremat.reshape(-1)), ("positive", scoremat[pos]), ("negative", scoremat[~pos])):
        out[name] = dict(highest=float(np.max(x)), lowest=float(np.min(x)), mean=float(np.mean(x)), variance=float(np.var(x)))
    u = usable_all_pairs(scoremat, spk(modelset), spk(segset), skip_diagonal=False, upper_only=True)
    fp, fn = hardest(u, k)
    out["false_pos"] = confusable_pairs(fp, modelset, segset)
    out["false_neg"] = confusable_pairs(fn, modelset, segset)
    return out
