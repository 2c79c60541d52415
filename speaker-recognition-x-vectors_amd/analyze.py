"""Analyse trial scores on the GPU: moments, histograms and the hardest trials (include/xvec_analyze.h).

What the reference's extra/compare_speaker_results.py does once the EER is known, to see why it is what it is: maximum,
minimum, mean and variance of all, of the target and of the non-target scores; the distributions of the rounded scores; the
highest-scoring non-target and the lowest-scoring target cells with the speaker pairs they belong to.  The score matrix
stays where `PldaScorer.score` left it; a few hundred numbers cross to the host.

    summ = score_summary(scoremat, trials, bins=Bins(first=-80, n_bins=170))     # ScoreSummary
    summ.target.mean, summ.nontarget.var, summ.all.max, summ.all.t_max
    grid, dens = summ.histogram.density("target")                                # the KDE of the rounded scores, on the host
    hard = hardest_all_pairs(scoremat, speaker_labels, upper_only=True, k=200)   # HardestTrials
    pairs, num_pairs, performance = confusable_pairs(hard.nontarget, modelset, segset)
    numbers = compare_speaker_results(scoremat, modelset, segset)                # every number the reference script prints

The hardest lists are ordered by the fp64 score itself, ties to the lower trial index: exact and the same from run to run.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, ptr as _p, sized_workspace, stream as _stream
from .evaluate import TrialList, _class_ids, score_vector_or_matrix, trial_args

__all__ = ["Bins", "ClassMoments", "ScoreHistogram", "ScoreSummary", "HardestTrials", "score_summary", "score_summary_all_pairs",
           "hardest_trials", "hardest_all_pairs", "confusable_pairs", "compare_speaker_results", "plan", "MAX_BINS", "MAX_K",
           "FLOOR", "RINT", "RECORD"]

# include/xvec_analyze.h
MAX_BINS = 4094
MAX_K = 2048
FLOOR, RINT = 0, 1
RECORD = np.dtype([("score", "<f8"), ("row", "<i4"), ("col", "<i4"), ("t", "<i8")])      # xvec_analyze_record
_CLASS_WORDS = 8             # xvec_analyze_class: three int64, five doubles
_STATS_WORDS = 3 * _CLASS_WORDS + 2

_check = checker(_hip.lib.xvec_analyze_last_error)


@dataclass
class Bins:
    """The lattice of a histogram: score s falls into bin R(s / width) - first, R = rint (ties to even) or floor.  The
    defaults with `first` and `n_bins` are the reference's np.rint(score)."""
    first: int
    n_bins: int
    width: float = 1.0
    rounding: int = RINT
    hist_copies: int = 0     # the LDS copies of the table per block; 0: the plan's choice

    def _struct(self):
        return _hip.AnalyzeBins(float(self.width), int(self.first), int(self.n_bins), int(self.rounding), int(self.hist_copies), 0)


@dataclass
class ClassMoments:
    """`var` is the population variance (np.var); t_min / t_max: the lowest trial index (row * n_cols + col for all pairs)
    whose score equals min / max.  An empty class: n = 0, the positions -1, the rest NaN."""
    n: int
    min: float
    max: float
    mean: float
    var: float
    t_min: int
    t_max: int
    sum: float


@dataclass
class ScoreHistogram:
    """counts per bin for the non-target and the target trials (int64 arrays) and their sum `all`; `values`: the score each
    bin stands for (label * width); under / over: (non-target, target) counts outside the lattice."""
    nontarget: np.ndarray
    target: np.ndarray
    values: np.ndarray
    under: tuple
    over: tuple
    bins: Bins

    @property
    def all(self):
        return self.nontarget + self.target

    def counts(self, which="all"):
        if which not in ("all", "target", "nontarget"):
            raise ValueError(f"which = {which!r}: one of 'all', 'target', 'nontarget'")
        return getattr(self, which)

    def density(self, which="all", gridsize=100, cut=3, bw="scott"):
        """(grid, density): the Gaussian kernel density estimate of the binned values -- every bin's value repeated as often
        as it was counted -- on `gridsize` points from min - cut h to max + cut h.  h = n^(-1/5) std(ddof=1) (Scott's rule in
        one dimension, scipy's and seaborn's default), or `bw` itself when it is a number.  For RINT bins of width 1 these are
        exactly the rounded scores the reference hands to sns.distplot.  Parity with seaborn's distplot itself is UNPINNED:
        seaborn and statsmodels are not installed where this was built; the estimate is checked against
        scipy.stats.gaussian_kde.  Runs on the host: a few thousand numbers."""
        c = self.counts(which).astype(np.float64)
        keep = c > 0
        v, c = self.values[keep], c[keep]
        n = c.sum()
        if n < 2 or len(v) < 2:
            raise ValueError("density: needs two trials in two different bins")
        mean = (v * c).sum() / n
        std = np.sqrt((c * (v - mean) ** 2).sum() / (n - 1))
        h = n ** (-0.2) * std if bw == "scott" else float(bw)
        if not h > 0:
            raise ValueError(f"density: the bandwidth {h} must be positive")
        grid = np.linspace(v.min() - cut * h, v.max() + cut * h, int(gridsize))
        z = (grid[:, None] - v[None, :]) / h
        return grid, (np.exp(-0.5 * z * z) * c[None, :]).sum(axis=1) / (n * h * np.sqrt(2.0 * np.pi))


@dataclass
class ScoreSummary:
    nontarget: ClassMoments
    target: ClassMoments
    all: ClassMoments
    n_nan: int
    n_bad_index: int
    histogram: ScoreHistogram = None


@dataclass
class HardestTrials:
    """`nontarget`: the highest-scoring non-target trials, `target`: the lowest-scoring target trials, the hardest first;
    numpy structured arrays (RECORD: score, row, col, t) of at most k records each."""
    nontarget: np.ndarray
    target: np.ndarray
    k: int
    n_nan: int
    n_bad_index: int


def plan(n_trials: int, n_bins: int = 0) -> dict:
    """What the library plans for `n_trials` (host only): tiles, blocks, the most tiles a block walks, the depth of the
    summation tree, the histogram's LDS copies, the default candidate cap, the trial count at which a block walks a second
    tile."""
    out = (C.c_int64 * 8)()
    _check(_hip.lib.xvec_analyze_plan_host(int(n_trials), int(n_bins), out))
    names = ("tiles", "blocks", "most_tiles", "sum_depth", "hist_copies", "max_copies", "cand_cap", "second_tile_from")
    return dict(zip(names, (int(x) for x in out)))


# ---------------------------------------------------------------- summary

def _ld(s: torch.Tensor) -> int:
    return s.stride(0) if s.shape[0] > 1 else max(s.stride(0), s.shape[1])


def _summary_workspace(n, n_bins, device, workspace):
    refusal = lambda: ValueError(f"{n} trials, {n_bins} bins: the trial count must lie in 1 .. 2^31 - 1, the bins in 0 .. {MAX_BINS}")
    return sized_workspace(_hip.lib.xvec_analyze_summary_workspace_bytes(int(n), int(n_bins)), refusal, device, workspace)


def _moments(words: np.ndarray) -> ClassMoments:
    i, d = words.view(np.int64), words
    return ClassMoments(int(i[0]), float(d[3]), float(d[4]), float(d[5]), float(d[6]), int(i[1]), int(i[2]), float(d[7]))


def _read_summary(stats, counts, bins) -> ScoreSummary:
    w = stats.cpu().numpy()                                                       # 208 bytes
    tail = w.view(np.int64)[3 * _CLASS_WORDS:]
    hist = None
    if bins is not None:
        c = counts.cpu().numpy()
        labels = np.arange(bins.first, bins.first + bins.n_bins, dtype=np.float64)
        hist = ScoreHistogram(c[0, 1:-1].copy(), c[1, 1:-1].copy(), labels * float(bins.width), (int(c[0, 0]), int(c[1, 0])),
                              (int(c[0, -1]), int(c[1, -1])), bins)
    cls = [_moments(w[k * _CLASS_WORDS:(k + 1) * _CLASS_WORDS]) for k in range(3)]
    return ScoreSummary(cls[0], cls[1], cls[2], int(tail[0]), int(tail[1]), hist)


def _check_bins(bins, what):
    if bins is None:
        return 0
    if not isinstance(bins, Bins):
        raise TypeError(f"{what}: bins must be a Bins or None")
    if not 1 <= int(bins.n_bins) <= MAX_BINS:
        raise ValueError(f"{what}: n_bins = {bins.n_bins} must lie in 1 .. {MAX_BINS}")
    return int(bins.n_bins)


def _run_summary(s, row, col, tgt, n, bins, workspace, pairs=None) -> ScoreSummary:
    """xvec_analyze_summary over device tensors as they are; `pairs` = (row_class, col_class, skip_diagonal, upper_only)
    switches to xvec_analyze_summary_all_pairs."""
    device = s.device
    n_bins = 0 if bins is None else int(bins.n_bins)
    ws = _summary_workspace(n, n_bins, device, workspace)
    stats = torch.empty(_STATS_WORDS, dtype=torch.float64, device=device)
    counts = torch.empty((2, n_bins + 2), dtype=torch.int64, device=device) if bins is not None else None
    b = None if bins is None else C.byref(bins._struct())
    with torch.cuda.device(device):
        if pairs is None:
            _check(_hip.lib.xvec_analyze_summary(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n, b,
                                                 stats.data_ptr(), _p(counts), ws.data_ptr(), ws.numel(), _stream(device)))
        else:
            rc, cc, skip, upper = pairs
            _check(_hip.lib.xvec_analyze_summary_all_pairs(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], rc.data_ptr(), cc.data_ptr(),
                                                           int(bool(skip)), int(bool(upper)), b, stats.data_ptr(), _p(counts),
                                                           ws.data_ptr(), ws.numel(), _stream(device)))
    return _read_summary(stats, counts, bins)


def score_summary(scoremat, trials, bins: Bins = None, workspace=None) -> ScoreSummary:
    """n, min, max, mean and variance of the non-target, the target and all trials of `trials` (a TrialList over the device
    score matrix, or the target flags of a score vector), and with `bins` their histograms.  Trials whose score is NaN or
    whose index lies outside the matrix are counted (n_nan, n_bad_index) and left out, as evaluate_trials leaves them out."""
    what = "score_summary"
    s = score_vector_or_matrix(scoremat, what)
    _check_bins(bins, what)
    row, col, tgt, n = trial_args(s, trials, what)
    return _run_summary(s, row, col, tgt, n, bins, workspace)


def _pair_classes(s, row_labels, col_labels, what):
    n_rows, n_cols = s.shape
    rc, cc = _class_ids(row_labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != n_rows or len(cc) != n_cols:
        raise ValueError(f"{what}: {len(rc)} row and {len(cc)} column labels for a {n_rows} x {n_cols} matrix")
    return torch.from_numpy(rc).to(s.device), torch.from_numpy(cc).to(s.device)


def score_summary_all_pairs(scoremat, row_labels, col_labels=None, skip_diagonal=True, upper_only=False, bins: Bins = None,
                            workspace=None) -> ScoreSummary:
    """Every cell of the score matrix as a trial, a target iff the labels of its row and column are equal.  `upper_only`
    keeps the cells with row < col: a matrix scored against itself is counted once per unordered pair."""
    what = "score_summary_all_pairs"
    s = score_vector_or_matrix(scoremat, what)
    _check_bins(bins, what)
    rcd, ccd = _pair_classes(s, row_labels, col_labels, what)
    return _run_summary(s, None, None, None, s.shape[0] * s.shape[1], bins, workspace, (rcd, ccd, skip_diagonal, upper_only))


# ---------------------------------------------------------------- hardest

def _run_hardest(s, row, col, tgt, n, k, cand_cap, workspace, pairs=None) -> HardestTrials:
    device = s.device
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k = {k} must lie in 1 .. {MAX_K}")
    refusal = lambda: ValueError(f"{n} trials, k = {k}, cand_cap = {cand_cap}: the trial count must lie in 1 .. 2^31 - 1, "
                                 f"cand_cap must be 0 or lie in k .. 65536")
    ws = sized_workspace(_hip.lib.xvec_analyze_hardest_workspace_bytes(int(n), int(k), int(cand_cap)), refusal, device, workspace)
    lists = torch.zeros((2, int(k), RECORD.itemsize), dtype=torch.uint8, device=device)
    counts = torch.empty(4, dtype=torch.int64, device=device)
    sel = _hip.AnalyzeSelect(int(k), int(cand_cap))
    with torch.cuda.device(device):
        if pairs is None:
            _check(_hip.lib.xvec_analyze_hardest(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n,
                                                 C.byref(sel), lists[0].data_ptr(), lists[1].data_ptr(), counts.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream(device)))
        else:
            rc, cc, skip, upper = pairs
            _check(_hip.lib.xvec_analyze_hardest_all_pairs(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], rc.data_ptr(), cc.data_ptr(),
                                                           int(bool(skip)), int(bool(upper)), C.byref(sel), lists[0].data_ptr(),
                                                           lists[1].data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                                           _stream(device)))
    f0, f1, n_nan, n_bad = counts.cpu().tolist()
    rec = lists.cpu().numpy().view(RECORD).reshape(2, int(k))                    # 2 k records of 24 bytes
    return HardestTrials(rec[0, :f0].copy(), rec[1, :f1].copy(), int(k), int(n_nan), int(n_bad))


def hardest_trials(scoremat, trials, k=200, cand_cap=0, workspace=None) -> HardestTrials:
    """The k highest-scoring non-target and the k lowest-scoring target trials of `trials` (as score_summary takes them).
    `cand_cap`: the candidate buffer of the select (0: the library's default)."""
    what = "hardest_trials"
    s = score_vector_or_matrix(scoremat, what)
    row, col, tgt, n = trial_args(s, trials, what)
    return _run_hardest(s, row, col, tgt, n, k, cand_cap, workspace)


def hardest_all_pairs(scoremat, row_labels, col_labels=None, skip_diagonal=True, upper_only=False, k=200, cand_cap=0,
                      workspace=None) -> HardestTrials:
    """hardest_trials over every cell of the matrix (score_summary_all_pairs says which cells)."""
    what = "hardest_all_pairs"
    s = score_vector_or_matrix(scoremat, what)
    rcd, ccd = _pair_classes(s, row_labels, col_labels, what)
    return _run_hardest(s, None, None, None, s.shape[0] * s.shape[1], k, cand_cap, workspace, (rcd, ccd, skip_diagonal, upper_only))


# ---------------------------------------------------------------- the reference's lists (host)

def _speaker(name) -> str:
    return str(name).split(".")[0].split("/")[0]


def _speaker_number(name) -> int:
    return int(str(name).split("/")[0][2:])          # 'id10304/...' -> 10304, as the reference reads it


def confusable_pairs(hardest, row_speakers, col_speakers):
    """(pairs, num_pairs, performance) as extra/compare_speaker_results.py:101-131 collects them for one list of hits
    (`hardest`: a record array, HardestTrials.nontarget or .target): the unordered speaker pairs in order of first appearance,
    the 1-based pair number of every hit, and the scores.  `row_speakers` / `col_speakers`: the ids of the matrix's rows and
    columns ('id10304/...': the number behind 'id' is the speaker), or speaker numbers themselves."""
    number = lambda x: int(x) if isinstance(x, (int, np.integer)) else _speaker_number(x)
    pairs, num_pairs, performance = [], [], []
    for r in hardest:
        a, b = sorted((number(row_speakers[int(r["row"])]), number(col_speakers[int(r["col"])])))
        if (a, b) not in pairs:
            pairs.append((a, b))
        num_pairs.append(pairs.index((a, b)) + 1)
        performance.append(float(r["score"]))
    return pairs, num_pairs, performance


def compare_speaker_results(scoremat, modelset, segset, k=100) -> dict:
    """Every number extra/compare_speaker_results.py prints, from the device score matrix: 'all', 'positive' and 'negative'
    each with highest, lowest, mean and variance -- computed the reference's way: a cell is positive iff the speaker prefixes of
    its two ids agree, and the diagonal takes part -- and 'false_pos' / 'false_neg': (pairs, num_pairs, performance) of the k
    hardest cells with row < col (the script walks 2 k hits of the two-sided matrix and prints every second one)."""
    what = "compare_speaker_results"
    s = score_vector_or_matrix(scoremat, what)
    rows, cols = [_speaker(m) for m in np.asarray(modelset).tolist()], [_speaker(x) for x in np.asarray(segset).tolist()]
    summ = score_summary_all_pairs(s, rows, cols, skip_diagonal=False)
    hard = hardest_all_pairs(s, rows, cols, skip_diagonal=False, upper_only=True, k=k)
    out = {}
    for name, m in (("all", summ.all), ("positive", summ.target), ("negative", summ.nontarget)):
        out[name] = dict(highest=m.max, lowest=m.min, mean=m.mean, variance=m.var)
    out["false_pos"] = confusable_pairs(hard.nontarget, modelset, segset)
    out["false_neg"] = confusable_pairs(hard.target, modelset, segset)
    return out
