"""Speaker identification on the GPU: models enrolled from several vectors, open-set scores, the k best models of every
test segment (include/xvec_ident.h).

The reference scores every utterance under its own id with `p_known=0.0`; these are the two other branches of the call it
makes, speechbrain's `fast_PLDA_scoring` (per-model averaging of the enrolment vectors, `mean_stat_per_model`; the open-set
correction for `p_known != 0`), and the decision an identification system takes behind them.  Parity with speechbrain
itself is unpinned (not installed in the build image); the kernels are checked against tests/ident_ref.py, numpy
restatements of the package's published code.  The score matrices stay where `PldaScorer.score` / `cosine_scores` left them.

    models = enroll(xvecs, names)                       # SpeakerModels: .names (sorted, unique), .vectors [M, D] on the device
    S = scorer.score(models.vectors, test_xvecs)        # ordinary x-vectors: PldaScorer, cosine_scores, ScoreNormalizer
    S = open_set_scores(S, p_known=0.1)                 # S - log(p mean over the OTHER models of exp S + (1 - p))
    idx, val, decision = identify(S, k=5, threshold=0.0)        # [k, T] int32 / float64, best first; [T] int32, -1 = nobody

    ident = SpeakerIdentifier(scorer, models)           # or SpeakerIdentifier("cosine", models)
    res = ident.identify(test_xvecs, k=5, p_known=0.1, threshold=0.0)    # nothing crosses to the host
    rank1, rankk = identification_rate(res.idx, true_model_index)

Equal scores are ordered by the lower model index, NaN is never selected, places that cannot be filled hold index -1 and
score NaN.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, dev_f64, i64_ptr, require_device, score_matrix, stream as _stream

__all__ = ["group_models", "SpeakerModels", "enroll", "open_set_scores", "identify", "Identification", "SpeakerIdentifier",
           "identification_rate", "COLS", "SLICE_ROWS", "BLOCK_ROWS", "TOPK_BLOCK_ROWS", "APPLY_ROWS", "APPLY_COLS", "MAX_K"]

# include/xvec_ident.h: the columns and rows of a wave's slice, the rows a block of the column statistics and of the top-k
# walk covers, the tile of the open-set pass, the longest list
COLS, SLICE_ROWS, BLOCK_ROWS, TOPK_BLOCK_ROWS, APPLY_ROWS, APPLY_COLS, MAX_K = 64, 32, 128, 512, 8, 256, 16

_check = checker(_hip.lib.xvec_ident_last_error)


def group_models(names):
    """(unique_names, order, model_start) of one model name per enrolment vector: the sorted unique names (np.unique, as
    StatObject_SB.mean_stat_per_model lists the models), `order` (int32) a stable permutation that groups the vectors by
    model, and `model_start` (int64, M + 1) the offsets of the models in it: model c owns order[model_start[c] :
    model_start[c + 1]], in the order the vectors were given.  Host only."""
    names = np.asarray(names)
    if names.ndim != 1 or names.shape[0] < 1:
        raise ValueError("group_models: expected one model name per vector (a non-empty 1-d sequence)")
    unique, inverse, counts = np.unique(names, return_inverse=True, return_counts=True)
    order = np.argsort(inverse.reshape(-1), kind="stable").astype(np.int32)
    start = np.zeros(unique.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=start[1:])
    return unique, order, start


class SpeakerModels(NamedTuple):
    names: np.ndarray          # [M] the sorted unique model names
    vectors: torch.Tensor      # [M, D] float64 on the device: ordinary x-vectors
    counts: np.ndarray         # [M] int64: enrolment vectors per model


def enroll(xvecs, names, device="cuda:0") -> SpeakerModels:
    """One x-vector per speaker model: the plain mean of the rows of `xvecs` [n, D] (array or tensor, float32 or float64; a
    device tensor with a row stride is read where it is) whose entry of `names` is the model's."""
    device = require_device(device, "enrolment")
    unique, order, start = group_models(names)
    if isinstance(xvecs, torch.Tensor) and xvecs.device == device and xvecs.dim() == 2 and xvecs.stride(1) == 1 \
            and xvecs.stride(0) >= xvecs.shape[1] and xvecs.dtype in (torch.float32, torch.float64):
        x = xvecs.detach()
    else:
        x = dev_f64(xvecs, device, keep_f32=True)
    if x.dim() != 2 or x.shape[0] != order.shape[0] or x.shape[1] < 1:
        raise ValueError(f"enroll: {order.shape[0]} names for x-vectors of shape {tuple(x.shape)}")
    n, dim, m = int(x.shape[0]), int(x.shape[1]), int(unique.shape[0])
    out = torch.empty((m, dim), dtype=torch.float64, device=device)
    order_d = torch.from_numpy(order).to(device)
    ws = byte_workspace(_hip.lib.xvec_model_mean_workspace_bytes(m), device)
    xd = _hip.IDENT_X_F32 if x.dtype == torch.float32 else _hip.IDENT_X_F64
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_model_mean(x.data_ptr(), xd, n, dim, x.stride(0), order_d.data_ptr(), i64_ptr(start), m,
                                        out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(device)))
    return SpeakerModels(unique, out, np.diff(start))


def _matrix(scores, what) -> torch.Tensor:
    return score_matrix(scores, what, "[n_models, n_tests]")


def open_set_scores(S, p_known, out=None, workspace=None) -> torch.Tensor:
    """out[i, j] = S[i, j] - log(p_known * mean over the models k != i of exp(S[k, j]) + (1 - p_known)) of the device score
    matrix S [N models, T tests] (float64, N >= 2, 0 < p_known <= 1): fast_PLDA_scoring's open-set scores.  `out=S` works in
    place."""
    in_place = out is S
    s = _matrix(S, "open_set_scores")
    if in_place and s is not S:
        raise ValueError("open_set_scores: in place needs a score matrix with unit column stride")
    n, t = s.shape
    p_known = float(p_known)
    if n < 2:
        raise ValueError("open_set_scores: need at least two models")
    if not 0.0 < p_known <= 1.0:
        raise ValueError(f"open_set_scores: p_known = {p_known} must lie in (0, 1]")
    if in_place:
        out = s
    elif out is None:
        out = torch.empty((n, t), dtype=torch.float64, device=s.device)
    elif (not isinstance(out, torch.Tensor) or out.device != s.device or out.dtype != torch.float64 or out.shape != s.shape
          or out.stride(1) != 1 or out.stride(0) < t):
        raise ValueError("open_set_scores: out must be a float64 device matrix of the scores' shape with unit column stride")
    ws = byte_workspace(int(_hip.lib.xvec_ident_workspace_bytes(n, t, 0)), s.device, workspace)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_open_set_scores(s.data_ptr(), s.stride(0), n, t, p_known, out.data_ptr(), out.stride(0),
                                             ws.data_ptr(), ws.numel(), _stream(s.device)))
    return out


class Identification(NamedTuple):
    idx: torch.Tensor                    # [k, T] int32: row r = the r-th best model of every test column, -1 = none
    scores: torch.Tensor                 # [k, T] float64: its score, NaN where idx is -1
    decision: Optional[torch.Tensor]     # [T] int32: the best model if its score >= threshold, else -1; None without a threshold


def identify(S, k=1, threshold=None, workspace=None) -> Identification:
    """The k best models (rows) of every test column of the device score matrix S [N, T], best first; equal scores by lower
    model index, NaN never.  With a `threshold` also the decision per column: the best model, or -1 (out of set) when its score
    is below the threshold."""
    s = _matrix(S, "identify")
    n, t = s.shape
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"identify: k = {k} must lie in 1 .. {MAX_K}")
    idx = torch.empty((k, t), dtype=torch.int32, device=s.device)
    val = torch.empty((k, t), dtype=torch.float64, device=s.device)
    decision = None if threshold is None else torch.empty(t, dtype=torch.int32, device=s.device)
    ws = byte_workspace(int(_hip.lib.xvec_ident_workspace_bytes(n, t, k)), s.device, workspace)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_identify_topk(s.data_ptr(), s.stride(0), n, t, k, 0.0 if threshold is None else float(threshold),
                                           idx.data_ptr(), val.data_ptr(), None if decision is None else decision.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(s.device)))
    return Identification(idx, val, decision)


class SpeakerIdentifier:
    """Enrolled models behind one scorer on one HIP device.  `scorer`: a `PldaScorer` or the string "cosine"; `models`: a
    `SpeakerModels` (or anything with `.names` and `.vectors`); `normalizer`: an optional `ScoreNormalizer` built over the same
    scorer, whose S-norm is applied between scoring and the open-set step."""

    def __init__(self, scorer, models, normalizer=None, device="cuda:0"):
        self.device = require_device(device, "identification")
        if isinstance(scorer, str):
            if scorer != "cosine":
                raise ValueError(f"SpeakerIdentifier: unknown scorer {scorer!r} (a PldaScorer or 'cosine')")
        elif not hasattr(scorer, "score"):
            raise TypeError("SpeakerIdentifier: scorer must be a PldaScorer or the string 'cosine'")
        elif torch.device(scorer.device) != self.device:
            raise ValueError(f"SpeakerIdentifier: the scorer lives on {scorer.device}, not on {self.device}")
        self.scorer = scorer
        self.names = np.asarray(models.names)
        self.vectors = dev_f64(models.vectors, self.device)
        if self.vectors.dim() != 2 or self.vectors.shape[0] != self.names.shape[0]:
            raise ValueError("SpeakerIdentifier: models.vectors must be [M, D] with one row per name")
        self.normalizer = normalizer
        self._ws = None

    def scores(self, test_xvecs, p_known=0.0) -> torch.Tensor:
        """The [M, T] device score matrix the decision is taken on: raw, S-normalised if a normalizer was given, open-set if
        p_known != 0."""
        t = dev_f64(test_xvecs, self.device)
        if self.scorer == "cosine":
            from .scoring import cosine_scores
            s = cosine_scores(self.vectors, t, device=self.device)
        else:
            s = self.scorer.score(self.vectors, t)
        if self.normalizer is not None:
            s = self.normalizer.normalize(s, self.vectors, t, mode="s", out=s)
        if p_known != 0:
            self._ws = byte_workspace(int(_hip.lib.xvec_ident_workspace_bytes(s.shape[0], s.shape[1], MAX_K)), self.device,
                                      self._ws)
            s = open_set_scores(s, p_known, out=s, workspace=self._ws)
        return s

    def identify(self, test_xvecs, k=1, p_known=0.0, threshold=None) -> Identification:
        s = self.scores(test_xvecs, p_known)
        self._ws = byte_workspace(int(_hip.lib.xvec_ident_workspace_bytes(s.shape[0], s.shape[1], MAX_K)), self.device, self._ws)
        return identify(s, k, threshold, workspace=self._ws)


def identification_rate(idx, truth):
    """(rank-1, rank-k) hit rates of `idx` [k, T] (what `identify` returns) against `truth` [T], the index of every test
    segment's true model: the share of segments whose true model is the best one, and is among the k listed."""
    idx_t = torch.as_tensor(idx)
    truth_t = torch.as_tensor(np.asarray(truth) if not isinstance(truth, torch.Tensor) else truth).to(idx_t.device)
    if idx_t.dim() != 2 or truth_t.shape != (idx_t.shape[1],):
        raise ValueError("identification_rate: idx must be [k, T] and truth [T]")
    hit = idx_t.to(torch.int64) == truth_t.to(torch.int64)[None, :]
    return float(hit[0].double().mean()), float(hit.any(dim=0).double().mean())
