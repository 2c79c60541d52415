"""Bootstrap confidence intervals for EER and minDCF on the GPU (include/xvec_boot.h).

`evaluate_trials` ends in a point estimate; this module says how far it moves when the speakers of the test set change.  The
groups (speakers) of the two trial sides are resampled with replacement `n_boot` times, the trial list is re-evaluated under
every resample on the device, and percentiles of the replicates give the interval.  A resample changes the weight of a trial,
not the order of the scores: the trials are sorted once and every replicate is a weighted sweep over that order.  Only the
counters and two order statistics cross to the host.

    boot = bootstrap_trials(scoremat, trials, row_groups=speaker_of_row, col_groups=speaker_of_col, joint=True, n_boot=1000)
    boot.point.eer, boot.interval("eer"), boot.stderr("min_dcf")
    boot = bootstrap_all_pairs(scoremat, speaker_labels)              # the labels are the groups
    cmp = compare(boot_a, boot_b, "eer")                              # paired: same seed, same groups, same resamples

Without groups (and for a plain score vector) every trial is its own unit and gets a Poisson(1) weight: the Poisson
bootstrap, not a resample of fixed size.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, ptr as _p, sized_workspace, stream as _stream
from .evaluate import TrialList, TrialResult, _class_ids, score_vector_or_matrix, trial_args

__all__ = ["BootstrapResult", "BootstrapComparison", "bootstrap_trials", "bootstrap_all_pairs", "compare", "percentile_ranks",
           "group_counts", "poisson_weight", "MAX_GROUPS", "MAX_BOOT"]

# include/xvec_boot.h
MAX_GROUPS = 16384
MAX_BOOT = 100000
_RECORD_WORDS = 8            # xvec_boot_record: six doubles, two int64
_SUMMARY_WORDS = 5           # xvec_boot_summary: five int64
METRICS = ("eer", "min_dcf", "eer_threshold", "min_dcf_threshold", "far", "frr")

_check = checker(_hip.lib.xvec_boot_last_error)


def percentile_ranks(m: int, level: float):
    """The 1-based ranks (k_lo, k_hi) of the percentile interval among m sorted values: with alpha = (1 - level) / 2,
    k_lo = max(1, floor((m + 1) alpha)) and k_hi = m + 1 - k_lo (1000 values at 95 %: the 25th and the 976th)."""
    if m < 1:
        raise ValueError("no replicate to take a percentile of")
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} must lie inside (0, 1)")
    k_lo = max(1, math.floor((m + 1) * (1.0 - level) / 2.0 + 1e-9))
    return k_lo, m + 1 - k_lo


def _interval(values: torch.Tensor, level: float):
    v = values[~torch.isnan(values)]
    k_lo, k_hi = percentile_ranks(int(v.numel()), level)
    s = torch.sort(v).values
    lo, hi = s[torch.tensor([k_lo - 1, k_hi - 1], device=s.device)].tolist()      # the two numbers that cross to the host
    return lo, hi


@dataclass
class BootstrapResult:
    """`point`: the estimate on the list itself.  The tensors (device, length n_boot) hold the replicates 1 .. n_boot; a
    replicate that could not be evaluated (counted in n_degenerate / n_overflow) is NaN in the float tensors."""
    point: TrialResult
    eer: torch.Tensor
    min_dcf: torch.Tensor
    eer_threshold: torch.Tensor
    min_dcf_threshold: torch.Tensor
    far: torch.Tensor
    frr: torch.Tensor
    n_target: torch.Tensor
    n_nontarget: torch.Tensor
    n_nan: int
    n_bad_index: int
    n_bad_group: int
    n_degenerate: int
    n_overflow: int
    # what the run was drawn with
    n_boot: int
    seed: int
    mode: str                    # "rows", "cols", "independent", "joint" or "poisson"
    n_row_groups: int
    n_col_groups: int
    c_miss: float = 1.0
    c_fa: float = 1.0
    p_target: float = 0.5
    records: torch.Tensor = field(default=None, repr=False)      # [n_boot + 1, 8] float64 as the device wrote them

    def values(self, metric="eer") -> torch.Tensor:
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: one of {METRICS}")
        return getattr(self, metric)

    def interval(self, metric="eer", level=0.95):
        """The percentile interval (lo, hi) of `metric` over the replicates that are not NaN: of those m values in ascending
        order, the k_lo-th and the k_hi-th, k_lo = max(1, floor((m + 1)(1 - level) / 2)), k_hi = m + 1 - k_lo (1-based)."""
        return _interval(self.values(metric), level)

    def stderr(self, metric="eer") -> float:
        """The bootstrap standard error: the sample standard deviation (n - 1) of the replicates that are not NaN."""
        v = self.values(metric)
        v = v[~torch.isnan(v)]
        if v.numel() < 2:
            raise ValueError("stderr needs two replicates that are not NaN")
        return float(torch.std(v, unbiased=True))

    def drawn_with(self):
        return (self.seed, self.n_boot, self.mode, self.n_row_groups, self.n_col_groups)


@dataclass
class BootstrapComparison:
    """a - b of `metric`: at the point, the percentile interval of the per-replicate differences, and the share of the
    replicates (of those evaluated in both) in which a is strictly lower."""
    metric: str
    difference: float
    lo: float
    hi: float
    share_a_lower: float
    n_valid: int


def compare(a: BootstrapResult, b: BootstrapResult, metric="eer", level=0.95) -> BootstrapComparison:
    """The paired comparison of two systems bootstrapped over the same resamples (same seed, n_boot, mode and group counts;
    anything else is refused: the differences would pair unrelated resamples)."""
    for name, x, y in (("seed", a.seed, b.seed), ("n_boot", a.n_boot, b.n_boot), ("mode", a.mode, b.mode),
                       ("group counts", (a.n_row_groups, a.n_col_groups), (b.n_row_groups, b.n_col_groups))):
        if x != y:
            raise ValueError(f"compare: the results differ in {name} ({x!r} and {y!r}): their replicates are not paired")
    d = a.values(metric) - b.values(metric).to(a.values(metric).device)
    valid = ~torch.isnan(d)
    n_valid = int(valid.sum())
    lo, hi = _interval(d, level)
    share = float((d[valid] < 0).double().mean())
    point = {"eer": "eer", "min_dcf": "min_dcf", "eer_threshold": "eer_th", "min_dcf_threshold": "min_dcf_th", "far": "far",
             "frr": "frr"}[metric]
    return BootstrapComparison(metric, getattr(a.point, point) - getattr(b.point, point), lo, hi, share, n_valid)


# ---------------------------------------------------------------- host entry points (no GPU)

def group_counts(seed: int, b: int, side: int, n_groups: int) -> np.ndarray:
    """The count table c_s,b [n_groups] of (seed, b, side) as the device draws it (uint16)."""
    out = np.zeros(max(1, int(n_groups)), dtype=np.uint16)
    _check(_hip.lib.xvec_boot_counts_host(int(seed) & (2 ** 64 - 1), int(b), int(side), int(n_groups),
                                          out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def poisson_weight(seed: int, b: int, t: int) -> int:
    """The Poisson(1) weight of trial t in replicate b."""
    w = C.c_int32(0)
    _check(_hip.lib.xvec_boot_poisson_host(int(seed) & (2 ** 64 - 1), int(b), int(t), C.byref(w)))
    return int(w.value)


# ---------------------------------------------------------------- the runs

def _mode(rg, cg, joint) -> str:
    if rg is None and cg is None:
        return "poisson"
    if joint:
        return "joint"
    return "independent" if rg is not None and cg is not None else ("rows" if rg is not None else "cols")


def _params(rg, cg, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target):
    return _hip.BootParams(_p(rg), _p(cg), int(g_rows), int(g_cols), int(bool(joint)), int(n_boot), int(seed) & (2 ** 64 - 1),
                           float(c_miss), float(c_fa), float(p_target))


def _workspace(n, n_boot, g_rows, g_cols, device, workspace):
    refusal = lambda: ValueError(f"{n} trials, n_boot = {n_boot}, {g_rows} and {g_cols} groups: the trial count must lie in "
                                 f"1 .. 2^31 - 1, n_boot in 1 .. {MAX_BOOT}, the groups of a side in 0 .. {MAX_GROUPS}")
    return sized_workspace(_hip.lib.xvec_boot_workspace_bytes(n, int(n_boot), int(g_rows), int(g_cols)), refusal, device,
                           workspace)


def _ld(s: torch.Tensor) -> int:
    """The row stride the library is told: torch's, except for a single row, whose stride may say anything."""
    return s.stride(0) if s.shape[0] > 1 else max(s.stride(0), s.shape[1])


def _result(records, summary, what, strict, n_boot, seed, mode, g_rows, g_cols, c_miss, c_fa, p_target) -> BootstrapResult:
    n_nan, n_bad, n_group, n_deg, n_over = summary.cpu().tolist()               # 40 bytes
    r0 = records[0].cpu()                                                       # and the point estimate: 64 bytes
    counts0 = r0.view(torch.int64)
    n_t, n_n = int(counts0[6]), int(counts0[7])
    if strict:
        if n_bad:
            raise IndexError(f"{what}: {n_bad} trial(s) point outside the score matrix")
        if n_group:
            raise IndexError(f"{what}: {n_group} trial(s) have a group id outside its range")
        if n_nan:
            raise ValueError(f"{what}: {n_nan} trial score(s) are NaN")
        if n_t == 0 or n_n == 0:
            raise ValueError(f"{what}: {n_t} target and {n_n} non-target trials; both kinds are needed")
    d = r0.tolist()
    point = TrialResult(d[0], d[1], d[2], d[3], d[4], d[5], n_t, n_n)
    reps, counts = records[1:], records.view(torch.int64)[1:]
    return BootstrapResult(point, reps[:, 0], reps[:, 4], reps[:, 1], reps[:, 5], reps[:, 2], reps[:, 3], counts[:, 6],
                           counts[:, 7], n_nan, n_bad, n_group, n_deg, n_over, int(n_boot), int(seed), mode, int(g_rows),
                           int(g_cols), float(c_miss), float(c_fa), float(p_target), records)


def _run_trials(s, row, col, tgt, n, rg, cg, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target, workspace, what,
                strict=True) -> BootstrapResult:
    """xvec_boot_trials over device tensors as they are (rg / cg: device int32 group ids or None)."""
    device = s.device
    ws = _workspace(n, n_boot, g_rows, g_cols, device, workspace)
    records = torch.empty((int(n_boot) + 1, _RECORD_WORDS), dtype=torch.float64, device=device)
    summary = torch.empty(_SUMMARY_WORDS, dtype=torch.int64, device=device)
    params = _params(rg, cg, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_boot_trials(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n,
                                         C.byref(params), summary.data_ptr(), records.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream(device)))
    return _result(records, summary, what, strict, n_boot, seed, _mode(rg, cg, joint), g_rows, g_cols, c_miss, c_fa, p_target)


def _run_all_pairs(s, rc, cc, skip_diagonal, rg, cg, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target, workspace, what,
                   strict=True) -> BootstrapResult:
    device = s.device
    n = s.shape[0] * s.shape[1]
    ws = _workspace(n, n_boot, g_rows, g_cols, device, workspace)
    records = torch.empty((int(n_boot) + 1, _RECORD_WORDS), dtype=torch.float64, device=device)
    summary = torch.empty(_SUMMARY_WORDS, dtype=torch.int64, device=device)
    params = _params(rg, cg, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_boot_all_pairs(s.data_ptr(), _ld(s), s.shape[0], s.shape[1], rc.data_ptr(), cc.data_ptr(),
                                            int(bool(skip_diagonal)), C.byref(params), summary.data_ptr(), records.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream(device)))
    return _result(records, summary, what, strict, n_boot, seed, _mode(rg, cg, joint), g_rows, g_cols, c_miss, c_fa, p_target)


def _group_ids(row_groups, col_groups, joint, n_rows, n_cols, what):
    """(row ids, col ids, G_rows, G_cols): host int32 ids compacted as evaluate._class_ids does it -- over one pool when joint."""
    if joint:
        if row_groups is None or col_groups is None:
            raise ValueError(f"{what}: joint needs row_groups and col_groups")
        rg, cg = _class_ids(row_groups, col_groups)
        g = int(max(rg.max(initial=-1), cg.max(initial=-1))) + 1
        g_rows = g_cols = g
    else:
        rg = None if row_groups is None else _class_ids(row_groups)[0]
        cg = None if col_groups is None else _class_ids(col_groups)[0]
        g_rows = 0 if rg is None else int(rg.max(initial=-1)) + 1
        g_cols = 0 if cg is None else int(cg.max(initial=-1)) + 1
    if rg is not None and len(rg) != n_rows or cg is not None and len(cg) != n_cols:
        raise ValueError(f"{what}: one group per row and per column of the {n_rows} x {n_cols} score matrix")
    if max(g_rows, g_cols) > MAX_GROUPS:
        raise ValueError(f"{what}: {g_rows} row and {g_cols} column groups: at most {MAX_GROUPS} on a side")
    return rg, cg, g_rows, g_cols


def _check_n_boot(n_boot, what):
    if not 1 <= int(n_boot) <= MAX_BOOT:
        raise ValueError(f"{what}: n_boot = {n_boot} must lie in 1 .. {MAX_BOOT}")


def bootstrap_trials(scoremat, trials, row_groups=None, col_groups=None, joint=False, n_boot=1000, seed=0, c_miss=1.0, c_fa=1.0,
                     p_target=0.5, workspace=None) -> BootstrapResult:
    """EER and minDCF of `trials` (a TrialList over the device score matrix, or the target flags of a score vector) with
    `n_boot` bootstrap replicates.  `row_groups` / `col_groups`: one label of any hashable kind per row / column of the matrix
    (the speaker of each enrolment model / test segment); either may be left out.  `joint=True` draws ONE resample over the
    pool of both sides' labels (enrolment and test speakers are the same people).  Without groups every trial is resampled on
    its own with a Poisson(1) weight."""
    what = "bootstrap_trials"
    s = score_vector_or_matrix(scoremat, what)
    _check_n_boot(n_boot, what)
    row, col, tgt, n = trial_args(s, trials, what)
    if row is None and (row_groups is not None or col_groups is not None):
        raise ValueError(f"{what}: a score vector has no sides to group; pass a TrialList over a matrix")
    rg, cg, g_rows, g_cols = _group_ids(row_groups, col_groups, joint, s.shape[0], s.shape[1], what)
    rgd = None if rg is None else torch.from_numpy(rg).to(s.device)
    cgd = None if cg is None else torch.from_numpy(cg).to(s.device)
    return _run_trials(s, row, col, tgt, n, rgd, cgd, g_rows, g_cols, joint, n_boot, seed, c_miss, c_fa, p_target, workspace, what)


def bootstrap_all_pairs(scoremat, row_labels, col_labels=None, skip_diagonal=True, n_boot=1000, seed=0, c_miss=1.0, c_fa=1.0,
                        p_target=0.5, workspace=None) -> BootstrapResult:
    """Every cell of the score matrix as a trial (evaluate_all_pairs) with `n_boot` replicates.  The labels themselves are
    the groups: speakers are resampled.  `col_labels=None` takes the row labels and is joint (one pool of speakers); with
    column labels the two sides are drawn independently."""
    what = "bootstrap_all_pairs"
    s = score_vector_or_matrix(scoremat, what)
    _check_n_boot(n_boot, what)
    n_rows, n_cols = s.shape
    joint = col_labels is None
    rc, cc = _class_ids(row_labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != n_rows or len(cc) != n_cols:
        raise ValueError(f"{what}: {len(rc)} row and {len(cc)} column labels for a {n_rows} x {n_cols} matrix")
    g = int(max(rc.max(), cc.max())) + 1          # the ids are shared between the sides: equal labels <-> equal ids
    if g > MAX_GROUPS:
        raise ValueError(f"{what}: {g} labels: at most {MAX_GROUPS} groups on a side")
    rcd, ccd = torch.from_numpy(rc).to(s.device), torch.from_numpy(cc).to(s.device)
    return _run_all_pairs(s, rcd, ccd, skip_diagonal, rcd, ccd, g, g, joint, n_boot, seed, c_miss, c_fa, p_target, workspace, what)
