"""Score fusion on the GPU: logistic fusion of several systems' scores and of quality measures (include/xvec_fuse.h).

Not in the reference.  What BOSARIS calls train_linear_fusion: the weights and the bias of llr = b + sum_k w_k f_k, fitted by
prior-weighted logistic regression on a development trial list.  A term f_k is a score matrix (PLDA, cosine, another
extractor, an S-normed matrix) or a quality measure of the row or of the column side, such as the logarithm of a segment's
duration.  The matrices stay where `PldaScorer.score` / `ScoreNormalizer.normalize` left them, and so do the weights:

    terms = [matrix(plda_scores), matrix(cos_scores), *log_duration_terms(enrol_frames, test_frames)]
    fus = fit_fusion(terms, dev_trials, p_target=0.01)               # Fusion: a device record, nothing synchronised
    llr = fus.apply(eval_terms)                                      # ((w0 f0 + w1 f1) + ...) + b, read on the device
    rep = calibration_report(llr, trials, p_target=0.01)             # the existing calls take the fused matrix
    fus.result()                                                     # FusionResult(weights, bias, objective_bits, ...)

    fuser = ScoreFuser(p_target=0.01).fit(terms, dev_trials)         # shaped like ScoreCalibrator
    llr = fuser.fuse(eval_terms)

There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import hip as _hip
from ._device import checker, ptr as _p, score_matrix, sized_workspace, stream as _stream
from .calibrate import DEFAULT_MAX_ITER
from .evaluate import TrialList, _class_ids, score_vector_or_matrix as _scores

__all__ = ["Term", "Fusion", "FusionResult", "ScoreFuser", "matrix", "row_quality", "col_quality", "log_duration_terms",
           "fit_fusion", "fit_fusion_all_pairs", "MAX_TERMS", "MATRIX", "ROW", "COL", "STEP_TOL", "CONVERGED", "MAX_ITER_REACHED",
           "ONE_CLASS", "INF_SCORE", "term_ulps"]

# include/xvec_fuse.h: the most terms, the kinds of a term, the stopping tolerance, the status codes of a fit
MAX_TERMS = 8
MATRIX, ROW, COL = 0, 1, 2
STEP_TOL = 1e-9
CONVERGED, MAX_ITER_REACHED, ONE_CLASS, INF_SCORE = 0, 1, 2, 3


def term_ulps(k: int) -> int:
    """XVEC_FUSE_TERM_ULPS(K)."""
    return 6 + (58 * (4 * int(k) + 1) + 4) // 5


_check = checker(_hip.lib.xvec_fuse_last_error)


class _Term(C.Structure):        # xvec_fuse_term
    _fields_ = [("data", C.c_void_p), ("ld", C.c_int64), ("kind", C.c_int32)]


class _Fit(C.Structure):         # xvec_fuse_result
    _fields_ = [("w", C.c_double * MAX_TERMS), ("b", C.c_double), ("objective_bits", C.c_double), ("penalty_bits", C.c_double),
                ("n_target", C.c_int64), ("n_nontarget", C.c_int64), ("n_nan", C.c_int64), ("n_bad_index", C.c_int64),
                ("n_terms", C.c_int16), ("n_iter", C.c_int16), ("status", C.c_int16), ("constant_mask", C.c_uint16)]


@dataclass
class Term:
    """One term of a fusion: `kind` MATRIX (a [n_rows, n_cols] float64 device matrix with unit column stride), ROW (a
    float64 device vector over the rows) or COL (one over the columns)."""
    kind: int
    data: torch.Tensor


@dataclass
class FusionResult:
    weights: list                # one per term; exactly 0.0 for a constant term
    bias: float
    objective_bits: float        # the data part of the objective / ln 2: Cllr of the fused scores at p_target = 0.5
    penalty_bits: float          # the ridge part
    n_iter: int
    status: int
    n_target: int
    n_nontarget: int
    n_nan: int
    n_bad_index: int
    constant_terms: list         # the indices of the terms that are constant over the trials kept


def matrix(scores) -> Term:
    """A score matrix as a term (a float64 device vector counts as the [1, n] matrix of the plain-vector trial form)."""
    return Term(MATRIX, _scores(scores, "fuse.matrix"))


def _quality(v, what) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): the measure must be a device tensor")
    if v.dim() != 1 or v.dtype != torch.float64 or v.numel() < 1:
        raise ValueError(f"{what}: expected a float64 vector, not empty")
    return v.contiguous()


def row_quality(v) -> Term:
    """A quality measure of the row (enrolment) side: f(i, j) = v[i]."""
    return Term(ROW, _quality(v, "fuse.row_quality"))


def col_quality(v) -> Term:
    """A quality measure of the column (test) side: f(i, j) = v[j]."""
    return Term(COL, _quality(v, "fuse.col_quality"))


def log_duration_terms(row_frames, col_frames, device=None):
    """(ROW term, COL term): log(frames) of the two sides as float64 device vectors, the terms of duration-aware calibration.
    `row_frames` / `col_frames`: frame counts (> 0), device tensors or host arrays (then `device` says where to)."""
    out = []
    for frames, make, side in ((row_frames, row_quality, "row_frames"), (col_frames, col_quality, "col_frames")):
        if not isinstance(frames, torch.Tensor):
            if device is None:
                raise ValueError(f"log_duration_terms: {side} is a host array: say which device")
            frames = torch.as_tensor(frames).to(device)
        elif device is not None:
            frames = frames.to(device)
        if not frames.is_cuda:
            raise RuntimeError("log_duration_terms runs on a HIP device only (no CPU path)")
        if frames.dim() != 1 or frames.numel() < 1:
            raise ValueError(f"log_duration_terms: {side} must be a vector, not empty")
        out.append(make(torch.log(frames.to(torch.float64))))
    return out[0], out[1]


def _shape(terms, what):
    """(terms as a list, n_rows, n_cols, device) after the checks of csrc/fuse_plan.h, one text per refusal."""
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"{what}: {len(terms)} terms: the count must lie in 1 .. {MAX_TERMS}")
    rows = cols = device = None
    for k, t in enumerate(terms):
        if not isinstance(t, Term):
            raise TypeError(f"{what}: term {k} is not a Term (build it with matrix, row_quality or col_quality)")
        if t.kind not in (MATRIX, ROW, COL):
            raise ValueError(f"{what}: term {k}: unknown kind {t.kind}")
        if not isinstance(t.data, torch.Tensor) or not t.data.is_cuda:
            raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): term {k} must be a device tensor")
        if t.data.dtype != torch.float64 or t.data.dim() != (2 if t.kind == MATRIX else 1) or t.data.numel() < 1:
            raise ValueError(f"{what}: term {k}: expected a float64 {'matrix' if t.kind == MATRIX else 'vector'}, not empty")
        if t.data.stride(-1) != 1 or (t.kind == MATRIX and t.data.stride(0) < t.data.shape[1]):
            raise ValueError(f"{what}: term {k}: unit column stride and a row stride of at least n_cols are needed")
        if device is None:
            device = t.data.device
        elif t.data.device != device:
            raise ValueError(f"{what}: term {k} lives on {t.data.device}, term 0 on {device}")
        r = t.data.shape[0] if t.kind != COL else None
        c = t.data.shape[-1] if t.kind != ROW else None
        if (r is not None and rows is not None and r != rows) or (c is not None and cols is not None and c != cols):
            raise ValueError(f"{what}: term {k} of shape {tuple(t.data.shape)} does not fit the [{rows}, {cols}] of the terms before it")
        rows = r if r is not None else rows
        cols = c if c is not None else cols
    if rows is None or cols is None:
        raise ValueError(f"{what}: the terms do not give the shape: a MATRIX term, or a ROW and a COL term, is needed")
    return terms, rows, cols, device


def _term_array(terms):
    arr = (_Term * len(terms))()
    for k, t in enumerate(terms):
        arr[k].data, arr[k].ld, arr[k].kind = t.data.data_ptr(), (t.data.stride(0) if t.kind == MATRIX else 0), t.kind
    return arr


def _workspace(n: int, k: int, device, workspace=None) -> torch.Tensor:
    refusal = lambda: ValueError(f"{n} trials of {k} terms: the counts must lie in 1 .. 2^31 - 1 and 1 .. {MAX_TERMS}")
    return sized_workspace(_hip.lib.xvec_fuse_workspace_bytes(n, k), refusal, device, workspace)


def _check_fit_args(p_target, l2, max_iter, what):
    if not 0.0 < float(p_target) < 1.0:
        raise ValueError(f"{what}: p_target = {p_target} must lie strictly between 0 and 1")
    if not 0.0 <= float(l2) < float("inf"):
        raise ValueError(f"{what}: l2 = {l2} must be finite and not negative")
    if not 1 <= int(max_iter) <= 1000:
        raise ValueError(f"{what}: max_iter = {max_iter} must lie in 1 .. 1000")


class Fusion:
    """A linear fusion llr = b + sum_k w_k f_k whose parameters live in a device record (xvec_fuse_result).  Nothing here
    synchronises but `result()`."""

    def __init__(self, record: torch.Tensor, n_terms: int):
        self.record = record
        self.n_terms = int(n_terms)

    @property
    def device(self):
        return self.record.device

    def result(self) -> FusionResult:
        """Synchronises and returns what the fit left."""
        r = _Fit.from_buffer_copy(self.record.cpu().numpy().tobytes())
        k = int(r.n_terms)
        return FusionResult([float(r.w[q]) for q in range(k)], r.b, r.objective_bits, r.penalty_bits, int(r.n_iter),
                            int(r.status), int(r.n_target), int(r.n_nontarget), int(r.n_nan), int(r.n_bad_index),
                            [q for q in range(k) if r.constant_mask >> q & 1])

    def apply(self, terms, out=None) -> torch.Tensor:
        """((w0 f0 + w1 f1) + ...) + b over the terms' whole matrix (numpy's result bit for bit); `out` may be the tensor of
        a MATRIX term: in place."""
        terms, rows, cols, device = _shape(terms, "Fusion.apply")
        if len(terms) != self.n_terms:
            raise ValueError(f"Fusion.apply: {len(terms)} terms for a fusion of {self.n_terms}")
        if device != self.record.device:
            raise ValueError(f"Fusion.apply: the terms live on {device}, the fusion on {self.record.device}")
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float64, device=device)
        elif (not isinstance(out, torch.Tensor) or out.device != device or out.dtype != torch.float64
                or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or out.stride(0) < cols):
            raise ValueError("Fusion.apply: out must be a float64 device matrix of the terms' shape with unit column stride")
        for k, t in enumerate(terms):
            if out.data_ptr() == t.data.data_ptr() and (t.kind != MATRIX or t.data.stride(0) != out.stride(0)):
                raise ValueError(f"Fusion.apply: out overlaps term {k}: in place needs a MATRIX term of the same row stride")
        with torch.cuda.device(device):
            _check(_hip.lib.xvec_fuse_apply(_term_array(terms), len(terms), rows, cols, self.record.data_ptr(), out.data_ptr(),
                                            out.stride(0), _stream(device)))
        return out


def _record(device) -> torch.Tensor:
    return torch.empty(C.sizeof(_Fit) // 8, dtype=torch.float64, device=device)


def fit_fusion(terms, trials, p_target=0.5, l2=0.0, max_iter=DEFAULT_MAX_ITER, workspace=None) -> Fusion:
    """The weights and the bias that minimise the prior-weighted logistic objective of `trials` (a TrialList over the terms'
    matrix; or, for terms of one row, the target flags alone), with the ridge l2 / 2 sum w'^2 on the standardised weights.
    The launch sequence is fixed by `max_iter` and the number of terms.  Does not synchronise: `.result()` does."""
    _check_fit_args(p_target, l2, max_iter, "fit_fusion")
    terms, rows, cols, device = _shape(terms, "fit_fusion")
    if isinstance(trials, TrialList):
        if len(trials) < 1:
            raise ValueError("fit_fusion: no trials")
        row, col, tgt = trials.on(device)
        n = len(trials)
    else:
        tgt = torch.as_tensor(trials).to(device=device).ne(0).to(torch.uint8).contiguous()
        if rows != 1 or tgt.dim() != 1 or tgt.numel() != cols:
            raise ValueError("fit_fusion: target flags alone go with terms of one row and their length (a TrialList indexes a matrix)")
        row, col, n = None, None, tgt.numel()
    ws = _workspace(n, len(terms), device, workspace)
    rec = _record(device)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_fuse_fit(_term_array(terms), len(terms), rows, cols, _p(row), _p(col), tgt.data_ptr(), n,
                                      float(p_target), float(l2), int(max_iter), rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream(device)))
    return Fusion(rec, len(terms))


def fit_fusion_all_pairs(terms, labels, col_labels=None, skip_diagonal=True, p_target=0.5, l2=0.0, max_iter=DEFAULT_MAX_ITER,
                         workspace=None) -> Fusion:
    """fit_fusion over every cell of the terms' matrix: a target iff the row's and the column's label are equal."""
    _check_fit_args(p_target, l2, max_iter, "fit_fusion_all_pairs")
    terms, rows, cols, device = _shape(terms, "fit_fusion_all_pairs")
    rc, cc = _class_ids(labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != rows or len(cc) != cols:
        raise ValueError(f"fit_fusion_all_pairs: {len(rc)} row and {len(cc)} column labels for terms of {rows} x {cols}")
    rc, cc = torch.from_numpy(rc).to(device), torch.from_numpy(cc).to(device)
    ws = _workspace(rows * cols, len(terms), device, workspace)
    rec = _record(device)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_fuse_fit_all_pairs(_term_array(terms), len(terms), rows, cols, rc.data_ptr(), cc.data_ptr(),
                                                int(bool(skip_diagonal)), float(p_target), float(l2), int(max_iter),
                                                rec.data_ptr(), ws.data_ptr(), ws.numel(), _stream(device)))
    return Fusion(rec, len(terms))


class ScoreFuser:
    """Fit on development trials, fuse evaluation terms: shaped like `ScoreCalibrator`.

        fuser = ScoreFuser(p_target=0.01).fit(dev_terms, dev_trials)      # or .fit_all_pairs(dev_terms, labels)
        llr = fuser.fuse(eval_terms)                                      # out=<a MATRIX term's tensor>: in place
    """

    def __init__(self, p_target=0.5, l2=0.0, max_iter=DEFAULT_MAX_ITER):
        _check_fit_args(p_target, l2, max_iter, "ScoreFuser")
        self.p_target = float(p_target)
        self.l2 = float(l2)
        self.max_iter = int(max_iter)
        self.fusion = None
        self._ws = None

    def _keep(self, n, k, device):
        self._ws = _workspace(n, k, device, self._ws if self._ws is not None and self._ws.device == device else None)
        return self._ws

    def fit(self, terms, trials):
        terms, rows, cols, device = _shape(terms, "ScoreFuser.fit")
        n = len(trials) if isinstance(trials, TrialList) else int(torch.as_tensor(trials).numel())
        self.fusion = fit_fusion(terms, trials, self.p_target, self.l2, self.max_iter, self._keep(n, len(terms), device))
        return self

    def fit_all_pairs(self, terms, labels, col_labels=None, skip_diagonal=True):
        terms, rows, cols, device = _shape(terms, "ScoreFuser.fit_all_pairs")
        self.fusion = fit_fusion_all_pairs(terms, labels, col_labels, skip_diagonal, self.p_target, self.l2, self.max_iter,
                                           self._keep(rows * cols, len(terms), device))
        return self

    def fuse(self, terms, out=None) -> torch.Tensor:
        if self.fusion is None:
            raise RuntimeError("ScoreFuser.fuse: call fit or fit_all_pairs first")
        return self.fusion.apply(terms, out)

    def result(self) -> FusionResult:
        if self.fusion is None:
            raise RuntimeError("ScoreFuser.result: call fit or fit_all_pairs first")
        return self.fusion.result()
