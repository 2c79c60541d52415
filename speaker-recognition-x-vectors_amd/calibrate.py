"""Score calibration on the GPU: linear logistic regression, Cllr, PAV minCllr (include/xvec_calib.h).

Not in the reference (plda_score_stat.py stops at EER and minDCF, which are properties of the score ORDER).  What turns a
PLDA, cosine or S-normalised score into a log-likelihood ratio is an affine map fitted by prior-weighted logistic regression
on a development trial list (BOSARIS: train_linear_calibration); Cllr measures how good the LLRs are, minCllr how good they
could be after the best monotone map, and the actual DCF what the Bayes threshold costs next to the minimum `evaluate_trials`
reports.  The score matrices stay where `PldaScorer.score` / `ScoreNormalizer.normalize` left them, and so do a and b:

    cal = fit_calibration(dev_scores, dev_trials, p_target=0.01)     # Calibration: a device record, nothing synchronised
    llr = cal.apply(scorer.score(enroll, test))                      # a * S + b, a and b read on the device
    rep = calibration_report(llr, trials, p_target=0.01)             # cllr, min_cllr, calibration loss, act_dcf, min_dcf
    cal.result()                                                     # FitResult(a, b, objective_bits, n_iter, status, ...)

    calibrator = ScoreCalibrator(p_target=0.01).fit(dev_scores, dev_trials)      # shaped like ScoreNormalizer
    llr = calibrator.calibrate(eval_scores)

There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, score_matrix, sized_workspace, stream as _stream
from .evaluate import TrialList, _class_ids, evaluate_trials, score_vector_or_matrix as _scores, trial_args as _trial_args

__all__ = ["Calibration", "FitResult", "CllrResult", "PavResult", "CalibrationReport", "ScoreCalibrator", "fit_calibration",
           "fit_calibration_all_pairs", "cllr", "cllr_all_pairs", "min_cllr", "pav_segments", "calibration_report", "THREADS",
           "ITEMS", "MAX_BLOCKS", "TERM_ULPS", "HULL_CHUNK", "HULL_FINAL", "APPLY_ROWS", "APPLY_COLS", "CONVERGED",
           "MAX_ITER_REACHED", "ONE_CLASS", "INF_SCORE"]

# include/xvec_calib.h: the block size, the trials a thread takes per round, the cap of the grid, the per-term error constant,
# the hull's chunk and final-level threshold, apply's tile; the status codes of a fit
THREADS, ITEMS, MAX_BLOCKS, TERM_ULPS, HULL_CHUNK, HULL_FINAL, APPLY_ROWS, APPLY_COLS = 256, 8, 1024, 64, 16, 256, 8, 256
CONVERGED, MAX_ITER_REACHED, ONE_CLASS, INF_SCORE = 0, 1, 2, 3
DEFAULT_MAX_ITER = 50

_check = checker(_hip.lib.xvec_calib_last_error)


class _Fit(C.Structure):         # xvec_calib_fit_result
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("objective_bits", C.c_double), ("n_target", C.c_int64),
                ("n_nontarget", C.c_int64), ("n_nan", C.c_int64), ("n_bad_index", C.c_int64), ("n_iter", C.c_int32),
                ("status", C.c_int32)]


class _Cllr(C.Structure):        # xvec_calib_cllr_result
    _fields_ = [("cllr", C.c_double), ("act_dcf", C.c_double), ("p_miss", C.c_double), ("p_fa", C.c_double),
                ("threshold", C.c_double), ("n_target", C.c_int64), ("n_nontarget", C.c_int64), ("n_nan", C.c_int64),
                ("n_bad_index", C.c_int64)]


class _Pav(C.Structure):         # xvec_calib_pav_result
    _fields_ = [("min_cllr", C.c_double), ("n_segments", C.c_int64), ("n_target", C.c_int64), ("n_nontarget", C.c_int64),
                ("n_left_out", C.c_int64)]


@dataclass
class FitResult:
    a: float
    b: float
    objective_bits: float
    n_iter: int
    status: int
    n_target: int
    n_nontarget: int
    n_nan: int
    n_bad_index: int


@dataclass
class CllrResult:
    cllr: float
    act_dcf: float
    p_miss: float
    p_fa: float
    threshold: float
    n_target: int
    n_nontarget: int
    n_nan: int
    n_bad_index: int


@dataclass
class PavResult:
    min_cllr: float
    n_segments: int
    n_target: int
    n_nontarget: int
    n_left_out: int
    k_end: np.ndarray            # [min(n_segments, capacity)] int64: trials up to the end of every segment
    tp_end: np.ndarray           # int64: targets up to it
    score: np.ndarray            # float32: the largest score of the segment
    llr: np.ndarray              # float64: the segment's LLR


@dataclass
class CalibrationReport:
    cllr: float
    min_cllr: float
    calibration_loss: float      # cllr - min_cllr
    act_dcf: float
    min_dcf: float
    eer: float
    n_target: int
    n_nontarget: int


def _record(struct, device) -> torch.Tensor:
    return torch.empty(C.sizeof(struct) // 8, dtype=torch.float64, device=device)


def _read(struct, record: torch.Tensor):
    return struct.from_buffer_copy(record.cpu().numpy().tobytes())


def _workspace(n: int, device, workspace=None) -> torch.Tensor:
    refusal = lambda: ValueError(f"{n} trials: the count must lie in 1 .. 2^31 - 1")
    return sized_workspace(_hip.lib.xvec_calib_workspace_bytes(n), refusal, device, workspace)


def _classes(s: torch.Tensor, row_labels, col_labels, what: str):
    rc, cc = _class_ids(row_labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != s.shape[0] or len(cc) != s.shape[1]:
        raise ValueError(f"{what}: {len(rc)} row and {len(cc)} column labels for a {s.shape[0]} x {s.shape[1]} matrix")
    return torch.from_numpy(rc).to(s.device), torch.from_numpy(cc).to(s.device)


def _p(t):
    return None if t is None else t.data_ptr()


class Calibration:
    """An affine map llr = a * score + b whose parameters live in a device record (xvec_calib_fit_result).  Nothing here
    synchronises but `result()`."""

    def __init__(self, record: torch.Tensor):
        self.record = record

    @property
    def device(self):
        return self.record.device

    def result(self) -> FitResult:
        """Synchronises and returns what the fit left: a, b, the objective in bits, the passes made, the status, the counts."""
        r = _read(_Fit, self.record)
        return FitResult(r.a, r.b, r.objective_bits, int(r.n_iter), int(r.status), int(r.n_target), int(r.n_nontarget),
                         int(r.n_nan), int(r.n_bad_index))

    def apply(self, scoremat, out=None) -> torch.Tensor:
        """a * scoremat + b on the device (numpy's result bit for bit); `out=scoremat` works in place."""
        in_place = out is scoremat
        s = score_matrix(scoremat, "Calibration.apply")
        if s.device != self.record.device:
            raise ValueError(f"Calibration.apply: the scores live on {s.device}, the calibration on {self.record.device}")
        if in_place and s is not scoremat:
            raise ValueError("Calibration.apply: in place needs a score matrix with unit column stride")
        n_rows, n_cols = s.shape
        if out is None:
            out = torch.empty((n_rows, n_cols), dtype=torch.float64, device=s.device)
        elif not in_place:
            if (not isinstance(out, torch.Tensor) or out.device != s.device or out.dtype != torch.float64
                    or out.shape != s.shape or out.stride(1) != 1 or out.stride(0) < n_cols):
                raise ValueError("Calibration.apply: out must be a float64 device matrix of the scores' shape with unit column stride")
        with torch.cuda.device(s.device):
            _check(_hip.lib.xvec_calib_apply(s.data_ptr(), s.stride(0), n_rows, n_cols, self.record.data_ptr(), out.data_ptr(),
                                             out.stride(0), _stream(s.device)))
        return out


def _check_fit_args(p_target, max_iter, what):
    if not 0.0 < float(p_target) < 1.0:
        raise ValueError(f"{what}: p_target = {p_target} must lie strictly between 0 and 1")
    if not 1 <= int(max_iter) <= 1000:
        raise ValueError(f"{what}: max_iter = {max_iter} must lie in 1 .. 1000")


def fit_calibration(scoremat, trials, p_target=0.5, max_iter=DEFAULT_MAX_ITER, workspace=None) -> Calibration:
    """The affine map that minimises the prior-weighted logistic objective of `trials` (a TrialList over the device score
    matrix; or the target flags of a device score vector).  The launch sequence is fixed by `max_iter`; the passes after
    convergence return at once.  Does not synchronise: `.result()` does."""
    _check_fit_args(p_target, max_iter, "fit_calibration")
    s = _scores(scoremat, "fit_calibration")
    row, col, tgt, n = _trial_args(s, trials, "fit_calibration")
    ws = _workspace(n, s.device, workspace)
    rec = _record(_Fit, s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_calib_fit(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n,
                                       float(p_target), int(max_iter), rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(s.device)))
    return Calibration(rec)


def fit_calibration_all_pairs(scoremat, labels, col_labels=None, skip_diagonal=True, p_target=0.5, max_iter=DEFAULT_MAX_ITER,
                              workspace=None) -> Calibration:
    """fit_calibration over every cell of the matrix: a target iff the row's and the column's label are equal."""
    _check_fit_args(p_target, max_iter, "fit_calibration_all_pairs")
    s = score_matrix(scoremat, "fit_calibration_all_pairs")
    rc, cc = _classes(s, labels, col_labels, "fit_calibration_all_pairs")
    ws = _workspace(s.shape[0] * s.shape[1], s.device, workspace)
    rec = _record(_Fit, s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_calib_fit_all_pairs(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], rc.data_ptr(), cc.data_ptr(),
                                                 int(bool(skip_diagonal)), float(p_target), int(max_iter), rec.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream(s.device)))
    return Calibration(rec)


def _cllr_result(rec) -> CllrResult:
    r = _read(_Cllr, rec)
    return CllrResult(r.cllr, r.act_dcf, r.p_miss, r.p_fa, r.threshold, int(r.n_target), int(r.n_nontarget), int(r.n_nan),
                      int(r.n_bad_index))


def cllr(llrs, trials, c_miss=1.0, c_fa=1.0, p_target=0.5, workspace=None) -> CllrResult:
    """Cllr and the actual DCF at the Bayes threshold of the trials' scores read as LLRs."""
    s = _scores(llrs, "cllr")
    row, col, tgt, n = _trial_args(s, trials, "cllr")
    ws = _workspace(n, s.device, workspace)
    rec = _record(_Cllr, s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_calib_cllr(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n,
                                        float(c_miss), float(c_fa), float(p_target), rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _stream(s.device)))
    return _cllr_result(rec)


def cllr_all_pairs(llrs, labels, col_labels=None, skip_diagonal=True, c_miss=1.0, c_fa=1.0, p_target=0.5,
                   workspace=None) -> CllrResult:
    s = score_matrix(llrs, "cllr_all_pairs")
    rc, cc = _classes(s, labels, col_labels, "cllr_all_pairs")
    ws = _workspace(s.shape[0] * s.shape[1], s.device, workspace)
    rec = _record(_Cllr, s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_calib_cllr_all_pairs(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], rc.data_ptr(), cc.data_ptr(),
                                                  int(bool(skip_diagonal)), float(c_miss), float(c_fa), float(p_target),
                                                  rec.data_ptr(), ws.data_ptr(), ws.numel(), _stream(s.device)))
    return _cllr_result(rec)


def pav_segments(scores, trials, capacity=None, workspace=None) -> PavResult:
    """Pool-adjacent-violators over the trials' fp32-rounded scores: minCllr and the segments of the monotone map, at most
    `capacity` of them (default: as many as there are trials, so all of them; `n_segments` is the full count either way)."""
    s = _scores(scores, "pav_segments")
    row, col, tgt, n = _trial_args(s, trials, "pav_segments")
    cap = n if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("pav_segments: capacity must not be negative")
    ws = _workspace(n, s.device, workspace)
    rec = _record(_Pav, s.device)
    k_end = torch.zeros(max(cap, 1), dtype=torch.int64, device=s.device)
    tp_end = torch.zeros(max(cap, 1), dtype=torch.int64, device=s.device)
    score = torch.zeros(max(cap, 1), dtype=torch.float32, device=s.device)
    llr = torch.zeros(max(cap, 1), dtype=torch.float64, device=s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_calib_min_cllr(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], _p(row), _p(col), tgt.data_ptr(), n,
                                            rec.data_ptr(), k_end.data_ptr(), tp_end.data_ptr(), score.data_ptr(), llr.data_ptr(),
                                            cap, ws.data_ptr(), ws.numel(), _stream(s.device)))
    r = _read(_Pav, rec)
    m = min(int(r.n_segments), cap)
    return PavResult(r.min_cllr, int(r.n_segments), int(r.n_target), int(r.n_nontarget), int(r.n_left_out),
                     k_end[:m].cpu().numpy(), tp_end[:m].cpu().numpy(), score[:m].cpu().numpy(), llr[:m].cpu().numpy())


def min_cllr(scores, trials, workspace=None) -> float:
    """Cllr after the best monotone map of the scores (PAV; no Laplace correction)."""
    return pav_segments(scores, trials, capacity=0, workspace=workspace).min_cllr


def calibration_report(llrs, trials: TrialList, c_miss=1.0, c_fa=1.0, p_target=0.5, workspace=None) -> CalibrationReport:
    """Cllr, minCllr, the calibration loss (their difference), the actual DCF at the Bayes threshold and `evaluate_trials`'
    minimum DCF and EER of one trial list over one device matrix of LLRs."""
    s = score_matrix(llrs, "calibration_report")
    ws = _workspace(len(trials), s.device, workspace)
    c = cllr(s, trials, c_miss, c_fa, p_target, ws)
    if c.n_bad_index:
        raise IndexError(f"calibration_report: {c.n_bad_index} trial(s) point outside the score matrix")
    if c.n_nan:
        raise ValueError(f"calibration_report: {c.n_nan} trial score(s) are NaN")
    if c.n_target == 0 or c.n_nontarget == 0:
        raise ValueError(f"calibration_report: {c.n_target} target and {c.n_nontarget} non-target trials; both kinds are needed")
    m = min_cllr(s, trials, ws)
    e = evaluate_trials(s, trials, c_miss, c_fa, p_target)
    return CalibrationReport(c.cllr, m, c.cllr - m, c.act_dcf, e.min_dcf, e.eer, c.n_target, c.n_nontarget)


class ScoreCalibrator:
    """Fit on development trials, apply to evaluation matrices: shaped like `ScoreNormalizer`.

        calibrator = ScoreCalibrator(p_target=0.01).fit(dev_scores, dev_trials)      # or .fit_all_pairs(dev_scores, labels)
        llr = calibrator.calibrate(eval_scores)                                       # out=eval_scores: in place
    """

    def __init__(self, p_target=0.5, max_iter=DEFAULT_MAX_ITER):
        _check_fit_args(p_target, max_iter, "ScoreCalibrator")
        self.p_target = float(p_target)
        self.max_iter = int(max_iter)
        self.calibration = None
        self._ws = None

    def _keep(self, n, device):
        self._ws = _workspace(n, device, self._ws if self._ws is not None and self._ws.device == device else None)
        return self._ws

    def fit(self, scoremat, trials):
        s = _scores(scoremat, "ScoreCalibrator.fit")
        n = len(trials) if isinstance(trials, TrialList) else int(torch.as_tensor(trials).numel())
        self.calibration = fit_calibration(s, trials, self.p_target, self.max_iter, self._keep(n, s.device))
        return self

    def fit_all_pairs(self, scoremat, labels, col_labels=None, skip_diagonal=True):
        s = score_matrix(scoremat, "ScoreCalibrator.fit_all_pairs")
        self.calibration = fit_calibration_all_pairs(s, labels, col_labels, skip_diagonal, self.p_target, self.max_iter,
                                                     self._keep(s.shape[0] * s.shape[1], s.device))
        return self

    def calibrate(self, scoremat, out=None) -> torch.Tensor:
        if self.calibration is None:
            raise RuntimeError("ScoreCalibrator.calibrate: call fit or fit_all_pairs first")
        return self.calibration.apply(scoremat, out)

    def result(self) -> FitResult:
        if self.calibration is None:
            raise RuntimeError("ScoreCalibrator.result: call fit or fit_all_pairs first")
        return self.calibration.result()
