"""The definitions of include/xvec_snorm.h restated in np.longdouble: sort the valid cells of a row descending, take k.  A plain
module like eer_ref.py; tests/test_snorm.py checks it against the definition written out by brute force, the GPU tests check
the kernels against it."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


class RowRef:
    """n_used [n] int, kth / mean / std [n] longdouble (NaN where k < 2), abs_mean [n] = sum |x| / k over the selection."""

    def __init__(self, n):
        self.n_used = np.zeros(n, dtype=np.int64)
        self.kth = np.full(n, np.nan, dtype=LD)
        self.mean = np.full(n, np.nan, dtype=LD)
        self.std = np.full(n, np.nan, dtype=LD)
        self.abs_mean = np.full(n, np.nan, dtype=LD)


def sorted_valid(scores, skip_col=None):
    """The valid cells of every row, descending: what row_stats selects from (pass it as `rows` to share it between calls)."""
    s = np.asarray(scores, dtype=np.float64)
    rows = []
    for i in range(s.shape[0]):
        valid = ~np.isnan(s[i])
        if skip_col is not None and 0 <= int(skip_col[i]) < s.shape[1]:
            valid[int(skip_col[i])] = False
        rows.append(np.sort(s[i][valid])[::-1])
    return rows


def row_stats(scores, top_k=0, skip_col=None, rows=None) -> RowRef:
    rows = sorted_valid(scores, skip_col) if rows is None else rows
    ref = RowRef(len(rows))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, x in enumerate(rows):
            k = x.size if top_k == 0 else min(int(top_k), x.size)
            ref.n_used[i] = k
            if k < 2:
                continue
            x = x[:k].astype(LD)
            ref.kth[i] = x[-1] + LD(0)                      # -0.0 -> +0.0
            ref.mean[i] = x.sum() / LD(k)
            ref.abs_mean[i] = np.abs(x).sum() / LD(k)
            ref.std[i] = np.sqrt(((x - ref.mean[i]) ** 2).sum() / LD(k - 1))
    return ref


def apply(scores, row=None, col=None):
    """out in longdouble from (mean, std) pairs of the rows and / or the columns."""
    s = np.asarray(scores, dtype=np.float64).astype(LD)
    w = LD(0.5) if row is not None and col is not None else LD(1)
    out = np.zeros_like(s)
    with np.errstate(all="ignore"):
        if row is not None:
            out = out + w * (s - np.asarray(row[0], dtype=LD)[:, None]) / np.asarray(row[1], dtype=LD)[:, None]
        if col is not None:
            out = out + w * (s - np.asarray(col[0], dtype=LD)[None, :]) / np.asarray(col[1], dtype=LD)[None, :]
    return out


def sum_roundings(k, C, threads=512, waves=8):
    """Roundings a selected cell's value can pass through on the way to the kernel's sum of k terms (csrc/snorm.hip): thread t
    adds its ceil(C / threads) cells in order (the first add, to 0.0, is exact), 6 butterfly steps join the wave's lanes, the
    waves' sums are added in wave order (waves - 1 adds), then the product of the m cells at the cut with the cut value and
    its add.  Cells that are not selected add nothing (x + 0.0 is exact) and the product is exact for m = 1, so the sum is a
    tree over k - m + 1 leaves (k - m adds) plus, for m >= 2, one product: at most k - 1 roundings on any path, which is what a
    plain left-to-right sum of the k terms has."""
    per_thread = -(-C // threads)
    return min(k - 1, (per_thread - 1) + 6 + (waves - 1) + 2)


def mean_bound(ref: RowRef, C):
    """|mean - ref| <= (sum_roundings + 1 for the division) u (sum |x| / k), with 1 % for the higher-order terms."""
    r = np.array([sum_roundings(int(k), C) + 1 for k in ref.n_used], dtype=np.float64)
    return 1.01 * r * U * ref.abs_mean.astype(np.float64)


def std_bound(ref: RowRef, C):
    """Relative bound on std: every term (x - mean)^2 carries 3 roundings (the difference, squared: twice; the product: once),
    the sum sum_roundings more, the division one; the square root halves all of that and adds one of its own.  On top, the
    error d of the mean the kernel subtracts: sum (x - m - d)^2 = sum (x - m)^2 + k d^2, relative k d^2 / ((k - 1) std^2) on
    the variance, half of it on std, with |d| <= mean_bound and sum |x| / k <= |mean| + std: (k u |mean| / std)^2 at most,
    the std share of d going into the 1 % margin."""
    r = np.array([(sum_roundings(int(k), C) + 4) / 2.0 + 1 for k in ref.n_used], dtype=np.float64)
    k = ref.n_used.astype(np.float64)
    with np.errstate(all="ignore"):
        ill = (k * U * np.abs(ref.mean.astype(np.float64)) / ref.std.astype(np.float64)) ** 2
    return 1.01 * r * U + ill
