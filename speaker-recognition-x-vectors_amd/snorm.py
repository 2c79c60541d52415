"""Score normalisation against a cohort on the GPU: Z-, T-, S- and AS-norm (include/xvec_snorm.h).

Not in the reference (plda_score_stat.py evaluates raw scores).  Raw PLDA and cosine scores shift and scale with the enrolment
and the test recording; what every x-vector system in use puts between scoring and the trial evaluation is a normalisation of
each score by the mean and standard deviation of its two sides' scores against a cohort -- all of them (S-norm) or the
`top_k` largest (adaptive S-norm).  The score matrices stay where `PldaScorer.score` / `cosine_scores` left them.

    norm = ScoreNormalizer(scorer, cohort_xvecs, top_k=300)          # the cohort is uploaded once
    S = norm.normalize(scorer.score(x_vecs), x_vecs)                 # the self case: one set of statistics, both sides
    S = norm.normalize(scorer.score(enroll, test), enroll, test, mode="s")      # "z": enrol side only, "t": test side only
    res = evaluate_trials(S, trials)

    st = cohort_stats(cohort_scores, top_k=300)                      # CohortStats(mean, std, kth, n_used), device tensors
    out = apply_norm(scores, row_stats=st_e, col_stats=st_t)         # 0.5 (s - me) / se + 0.5 (s - mt) / st

A row's statistics are a function of that row alone, bit for bit (the kernel's contract), so `ScoreNormalizer.stats` may score
and reduce the vectors in chunks of any size.  A standard deviation of 0 is not clamped: the normalised score is what IEEE 754
gives (inf or NaN).  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import hip as _hip
from ._device import byte_workspace, checker, dev_f64, ptr, require_device, score_matrix as _matrix, stream as _stream

__all__ = ["CohortStats", "cohort_stats", "apply_norm", "ScoreNormalizer", "THREADS", "RESIDENT_SMALL", "RESIDENT_MAX",
           "APPLY_ROWS", "APPLY_COLS"]

# include/xvec_snorm.h: the block size of the row kernel, the row lengths at which it changes its LDS image and at which it
# starts to stream the row, and apply's tile
THREADS, RESIDENT_SMALL, RESIDENT_MAX, APPLY_ROWS, APPLY_COLS = 512, 4096, 16384, 8, 256

_check = checker(_hip.lib.xvec_snorm_last_error)


class CohortStats(NamedTuple):
    mean: torch.Tensor       # [n] float64
    std: torch.Tensor        # [n] float64, unbiased
    kth: torch.Tensor        # [n] float64: the smallest selected score
    n_used: torch.Tensor     # [n] int32: the cells selected (min(top_k, valid cells))


def cohort_stats(cohort_scores, top_k=0, skip_col=None, workspace=None) -> CohortStats:
    """Mean, unbiased standard deviation and smallest member of the `top_k` largest cells of every row of the device matrix
    `cohort_scores` [n, C] (float64; `top_k=0`: every cell).  NaN cells and the cell `skip_col[i]` of row i (int tensor [n],
    -1 = none: a vector that is itself in the cohort) are left out; a row with fewer than two cells left gets NaN."""
    s = _matrix(cohort_scores, "cohort_stats")
    n, c = s.shape
    top_k = int(top_k)
    if top_k < 0:
        raise ValueError("cohort_stats: top_k must not be negative (0 = the whole cohort)")
    device = s.device
    skip = None
    if skip_col is not None:
        skip = torch.as_tensor(skip_col).to(device=device, dtype=torch.int32).contiguous()
        if skip.shape != (n,):
            raise ValueError(f"cohort_stats: skip_col must hold one column per row ({n}), got {tuple(skip.shape)}")
    need = int(_hip.lib.xvec_snorm_workspace_bytes(n, c))
    ws = byte_workspace(need, device, workspace)
    vals = torch.empty((3, n), dtype=torch.float64, device=device)
    n_used = torch.empty(n, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_snorm_row_stats(s.data_ptr(), s.stride(0), n, c, top_k, None if skip is None else skip.data_ptr(),
                                             vals[0].data_ptr(), vals[1].data_ptr(), vals[2].data_ptr(), n_used.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(device)))
    return CohortStats(vals[0], vals[1], vals[2], n_used)


def _pair(stats, n, device, what):
    if stats is None:
        return None, None
    mean, std = stats[0], stats[1]
    out = []
    for t in (mean, std):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"apply_norm: the {what} statistics must be device tensors (no CPU path)")
        t = t.to(device=device, dtype=torch.float64).contiguous()
        if t.shape != (n,):
            raise ValueError(f"apply_norm: {what} statistics of shape {tuple(t.shape)} for {n} {what}s")
        out.append(t)
    return out


def apply_norm(scores, row_stats=None, col_stats=None, out=None) -> torch.Tensor:
    """Z-norm (`row_stats` only), T-norm (`col_stats` only) or S-/AS-norm (both: the mean of the two) of the device score matrix;
    each `*_stats` a CohortStats or any (mean, std, ...) of device tensors.  `out=scores` normalises in place."""
    if row_stats is None and col_stats is None:
        raise ValueError("apply_norm: neither row nor column statistics")
    in_place = out is scores
    s = _matrix(scores, "apply_norm")
    if in_place and s is not scores:
        raise ValueError("apply_norm: in place needs a score matrix with unit column stride")
    n_rows, n_cols = s.shape
    rm, rs = _pair(row_stats, n_rows, s.device, "row")
    cm, cs = _pair(col_stats, n_cols, s.device, "column")
    if out is None:
        out = torch.empty((n_rows, n_cols), dtype=torch.float64, device=s.device)
    elif not in_place:
        if (not isinstance(out, torch.Tensor) or out.device != s.device or out.dtype != torch.float64
                or out.shape != s.shape or out.stride(1) != 1 or out.stride(0) < n_cols):
            raise ValueError("apply_norm: out must be a float64 device matrix of the scores' shape with unit column stride")
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_snorm_apply(s.data_ptr(), s.stride(0), n_rows, n_cols, ptr(rm), ptr(rs), ptr(cm), ptr(cs),
                                         out.data_ptr(), out.stride(0), _stream(s.device)))
    return out


class ScoreNormalizer:
    """A cohort prepared for normalising the scores of one scorer on one HIP device.  `scorer`: a `PldaScorer` or the string
    "cosine"; `cohort`: [C, D] x-vectors, uploaded once; `top_k=0` takes the whole cohort (S-norm), `top_k > 0` the top_k
    cohort scores of every vector (adaptive S-norm).  No cohort score matrix of more than `max_bytes` is ever held."""

    def __init__(self, scorer, cohort, top_k=0, device="cuda:0", max_bytes=256 << 20):
        self.device = require_device(device, "score normalisation")
        if isinstance(scorer, str):
            if scorer != "cosine":
                raise ValueError(f"ScoreNormalizer: unknown scorer {scorer!r} (a PldaScorer or 'cosine')")
        elif not hasattr(scorer, "score"):
            raise TypeError("ScoreNormalizer: scorer must be a PldaScorer or the string 'cosine'")
        elif torch.device(scorer.device) != self.device:
            raise ValueError(f"ScoreNormalizer: the scorer lives on {scorer.device}, not on {self.device}")
        self.scorer = scorer
        self.cohort = dev_f64(cohort, self.device)
        if self.cohort.dim() != 2 or self.cohort.shape[0] < 2:
            raise ValueError("ScoreNormalizer: the cohort must be [C, D] x-vectors with C >= 2")
        self.top_k = int(top_k)
        if self.top_k < 0:
            raise ValueError("ScoreNormalizer: top_k must not be negative")
        self.max_bytes = int(max_bytes)
        self._ws = None

    def _cohort_scores(self, x) -> torch.Tensor:
        if self.scorer == "cosine":
            from .scoring import cosine_scores
            return cosine_scores(x, self.cohort, device=self.device)
        return self.scorer.score(x, self.cohort)

    def chunk_rows(self) -> int:
        """Rows of one [chunk, C] cohort score matrix: as many as `max_bytes` holds, at least one."""
        return max(1, self.max_bytes // (8 * self.cohort.shape[0]))

    def stats(self, x, skip_col=None) -> CohortStats:
        """CohortStats of the vectors `x` [n, D] against the cohort; `skip_col[i]` names the cohort member that IS vector i."""
        x = dev_f64(x, self.device)
        if x.dim() != 2 or x.shape[1] != self.cohort.shape[1]:
            raise ValueError(f"ScoreNormalizer.stats: expected [n, {self.cohort.shape[1]}] x-vectors")
        n = x.shape[0]
        skip = None
        if skip_col is not None:
            skip = torch.as_tensor(skip_col).to(device=self.device, dtype=torch.int32).contiguous()
            if skip.shape != (n,):
                raise ValueError(f"ScoreNormalizer.stats: skip_col must hold one column per vector ({n})")
        step = self.chunk_rows()
        parts = []
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            self._ws = byte_workspace(int(_hip.lib.xvec_snorm_workspace_bytes(r1 - r0, self.cohort.shape[0])), self.device,
                                      self._ws)
            parts.append(cohort_stats(self._cohort_scores(x[r0:r1]), self.top_k, None if skip is None else skip[r0:r1],
                                      self._ws))
        if len(parts) == 1:
            return parts[0]
        return CohortStats(*(torch.cat([p[f] for p in parts]) for f in range(4)))

    def normalize(self, scoremat, enroll, test=None, mode="s", out=None) -> torch.Tensor:
        """The device score matrix [n_enroll, n_test] normalised: mode "z" by the enrolment side's cohort statistics, "t" by the
        test side's, "s" by both.  `test=None` is the self case (the matrix scores `enroll` against itself): the statistics are
        computed once and used on both sides.  `out=scoremat` normalises in place."""
        if mode not in ("z", "t", "s"):
            raise ValueError(f"ScoreNormalizer.normalize: mode {mode!r} (one of 'z', 't', 's')")
        s = _matrix(scoremat, "ScoreNormalizer.normalize")
        row = col = None
        if test is None:
            both = self.stats(enroll)
            row = both if mode in ("z", "s") else None
            col = both if mode in ("t", "s") else None
        else:
            if mode in ("z", "s"):
                row = self.stats(enroll)
            if mode in ("t", "s"):
                col = self.stats(test)
        return apply_norm(s, row, col, out)
