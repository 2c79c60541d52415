"""numpy restatement of the image half of the reference's plot_images (plda_score_stat.py:132-192) and of the DET curve, for the
tests of the trial report (include/xvec_report.h), in the project's own words as tests/eer_ref.py is.  The reference module
cannot be imported where the tests run (speechbrain and seaborn are absent), so no fixture is written from it.

Two rules are the header's, not the reference's: the range of the score matrix is that of its FINITE cells (numpy's min / max
would turn every image to NaN on one NaN cell), and a float image becomes uint8 as trunc(clamp(float32(x) * 255, 0, 255)) with
NaN -> 0 (what the TensorBoard writer does, restated from memory)."""
import numpy as np

GAP = 5
NAMES = ("score_matrix", "ground_truth", "ground_truth_scores", "prediction_eer_min_dcf", "correct_prediction_eer_min_dcf",
         "false_prediction_eer_min_dcf")


def masks(row_idx, col_idx, is_target, shape):
    """(positive_scores_mask, negative_scores_mask, bad trials): float64 maps SET to 1 (plda_score_stat.py:86-92); a trial with
    an index outside the matrix is counted and touches nothing."""
    row, col = np.asarray(row_idx, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    tgt = np.asarray(is_target).astype(bool)
    ok = (row >= 0) & (row < shape[0]) & (col >= 0) & (col < shape[1])
    pos, neg = np.zeros(shape), np.zeros(shape)
    pos[row[ok & tgt], col[ok & tgt]] = 1
    neg[row[ok & ~tgt], col[ok & ~tgt]] = 1
    return pos, neg, int((~ok).sum())


def finite_range(S):
    f = S[np.isfinite(S)]
    return (f.min(), f.max()) if f.size else (np.inf, -np.inf)


def normalised(S):
    """scoremat_norm: `-= min; /= max` in place, over the finite range."""
    with np.errstate(all="ignore"):
        v = np.array(S, dtype=np.float64)
        v -= finite_range(S)[0]
        top = finite_range(v)[1] if np.isfinite(v).any() else -np.inf
        v /= top
    return v


def to_u8(x):
    with np.errstate(all="ignore"):
        y = np.asarray(x, dtype=np.float64).astype(np.float32) * np.float32(255.0)
        y = np.where(np.isnan(y), np.float32(0.0), np.clip(y, np.float32(0.0), np.float32(255.0)))
    return np.trunc(y).astype(np.uint8)


def images(S, pos, neg, eer_th, min_dcf_th):
    """The six float64 images, as the reference builds them."""
    S = np.asarray(S, dtype=np.float64)
    R, C = S.shape
    with np.errstate(all="ignore"):
        norm = normalised(S)
        out = {}
        img = np.zeros((3, R, C))
        img[0] = img[1] = img[2] = norm
        out["score_matrix"] = img
        img = np.zeros((3, R, C))
        img[1], img[0] = pos, neg
        out["ground_truth"] = img
        img = np.zeros((3, R, C))
        img[1], img[0] = norm * pos, norm * neg
        out["ground_truth_scores"] = img
        checked_map = pos + neg
        checked = checked_map * S
        pp_e = np.where(checked >= eer_th, 1, 0) * checked_map
        pn_e = np.where(checked < eer_th, 1, 0) * checked_map
        pp_m = np.where(checked >= min_dcf_th, 1, 0) * checked_map
        pn_m = np.where(checked < min_dcf_th, 1, 0) * checked_map
        for name, w1, w0 in (("prediction_eer_min_dcf", 1.0, 1.0), ("correct_prediction_eer_min_dcf", pos, neg),
                             ("false_prediction_eer_min_dcf", neg, pos)):
            img = np.ones((3, R, 2 * C + GAP))
            img[1, :, :C] = pp_e * w1
            img[0, :, :C] = pn_e * w0
            img[1, :, -C:] = pp_m * w1
            img[0, :, -C:] = pn_m * w0
            img[2, :, :C] = 0
            img[2, :, -C:] = 0
            out[name] = img
    return out


def as_dtype(img, dtype):
    """A float64 image as the library stores it: float32 (rounded once) or uint8."""
    if dtype == np.uint8:
        return to_u8(img)
    with np.errstate(all="ignore"):
        return np.asarray(img).astype(np.float32)


def same(got, want):
    """Bit for bit, NaN equal to NaN of any payload."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.uint8:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---------------------------------------------------------------- the DET curve

def select(S, row_idx, col_idx, is_target):
    """(scores, target flags, n_nan, n_bad) of the trials kept: index inside the matrix, score not NaN."""
    S = np.asarray(S, dtype=np.float64)
    row, col = np.asarray(row_idx, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    tgt = np.asarray(is_target).astype(bool)
    ok = (row >= 0) & (row < S.shape[0]) & (col >= 0) & (col < S.shape[1])
    s = S[row[ok], col[ok]]
    keep = ~np.isnan(s)
    return s[keep], tgt[ok][keep], int((~keep).sum()), int((~ok).sum())


def det_points(scores, is_target):
    """(thr float32, tp int64, nn int64, P, N): one point per distinct float32 score, ascending (-0.0 counts as +0.0)."""
    with np.errstate(over="ignore"):
        s = np.asarray(scores, dtype=np.float64).astype(np.float32) + np.float32(0.0)
    tgt = np.asarray(is_target).astype(bool)
    thr = np.unique(s)
    tp = np.searchsorted(np.sort(s[tgt]), thr, side="right").astype(np.int64)
    nn = np.searchsorted(np.sort(s[~tgt]), thr, side="right").astype(np.int64)
    return thr, tp, nn, int(tgt.sum()), int((~tgt).sum())


def thin(thr, tp, nn, P, N, grid):
    """The points the thinned curve keeps: the first, the last, and every point at which floor(tp grid / P) or
    floor((N - nn) grid / N) differs from its value at the point before (int64: counts and grid below 2^31)."""
    if grid == 0 or len(thr) == 0:
        return thr, tp, nn
    tp64, nn64 = np.asarray(tp, dtype=np.int64), np.asarray(nn, dtype=np.int64)
    a = tp64 * grid // P if P > 0 else np.zeros_like(tp64)
    b = (N - nn64) * grid // N if N > 0 else np.zeros_like(nn64)
    keep = np.ones(len(thr), dtype=bool)
    keep[1:-1] = ((a[1:] != a[:-1]) | (b[1:] != b[:-1]))[:-1]
    return thr[keep], tp[keep], nn[keep]
