"""GMM-UBM on the GPU: diagonal-covariance EM, Baum-Welch statistics, relevance MAP and scores (include/xvec_gmm.h).

The comparison system of the reference: a universal background model trained by EM on MFCC frames, the per-utterance zeroth-
and first-order statistics (SIDEKIT's stat0 / stat1, what an i-vector extractor reads), MAP-adapted speaker models and the
log-likelihood-ratio scores of the classical GMM-UBM verifier.

    feats, utt = frames_of(mfcc, lengths)                  # a padded [B, T, D] batch, no copy
    ubm = fit_ubm(feats, 512, utt=utt, n_iter=10)          # DiagGmm; ubm.lower_bounds, ubm.n_iter_
    enrol = ubm.stats(enrol_feats, enrol_utt)              # GmmStats(n [U, C], f [U, C, D])
    test = ubm.stats(test_feats, test_utt)
    models = map_adapt(ubm, enrol, relevance=16.0)         # [M, C, D]
    scores = linear_scores(ubm, models, test)              # [M, U] float64 on the device: evaluate_trials, snorm, calibrate, ...
    exact = llr_scores(ubm, models, test_feats, test_utt)  # the exact average LLR, a host loop over the models

All arithmetic is fp64; features may be fp32 or fp64.  The N x C posterior matrix is never stored.  Frames with a non-finite
coefficient are left out and counted (`n_bad`).  Not built: the i-vector extractor, full covariances, k-means initialisation
and mixture splitting, delta features.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, dev_f64, i64_ptr, ptr as _p, require_device, sized_workspace, stream as _stream

__all__ = ["DiagGmm", "GmmStats", "fit_ubm", "map_adapt", "linear_scores", "llr_scores", "frames_of", "plan", "MAX_C", "MAX_D"]

# include/xvec_gmm.h
MAX_C = 4096
MAX_D = 256

_check = checker(_hip.lib.xvec_gmm_last_error)


def plan(n_total: int, C_: int, D: int, n_utts: int = 1, per_utt: bool = False, n_slices: int = 0) -> dict:
    """What the library plans (host only): the tiles, the slices of the global statistics, K and the blocks."""
    out = (C.c_int64 * 10)()
    _check(_hip.lib.xvec_gmm_plan_host(int(n_total), int(n_utts), int(C_), int(D), int(bool(per_utt)), int(n_slices), out))
    names = ("frame_tile", "comp_tile", "comp_tiles", "col_tiles", "slices", "slice_frames", "k_pad", "k_chunks", "slab_doubles",
             "blocks")
    return dict(zip(names, (int(x) for x in out)))


def frames_of(x: torch.Tensor, lengths):
    """(feats, utt) of a padded batch x [B, T, D] with `lengths` valid frames per row, as every function here takes them:
    feats is x seen as [B T, D] (no copy), utt = (b T, lengths).  What the padding holds is never read."""
    if x.dim() != 3:
        raise ValueError("frames_of: expected a padded batch [B, T, D]")
    B, T, D = x.shape
    lengths = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
    if lengths.shape[0] != B or (lengths < 0).any() or (lengths > T).any():
        raise ValueError(f"frames_of: need {B} lengths in 0 .. {T}")
    x = x if x.is_contiguous() else x.contiguous()
    return x.view(B * T, D), (np.arange(B, dtype=np.int64) * T, lengths)


class _Frames:
    """The xvec_gmm_frames of one call and everything it points to."""

    def __init__(self, feats, utt, D, what):
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
            raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): the features must be a device tensor")
        if feats.dim() == 3 and utt is None:
            feats, utt = frames_of(feats, [feats.shape[1]] * feats.shape[0])
        if feats.dim() != 2 or feats.shape[1] != D or feats.dtype not in (torch.float32, torch.float64) or feats.shape[0] < 1:
            raise ValueError(f"{what}: expected float32 or float64 features [rows, {D}]")
        if feats.stride(1) != 1 or (feats.shape[0] > 1 and feats.stride(0) < D):
            feats = feats.contiguous()
        self.x = feats
        rows = feats.shape[0]
        if utt is None:
            utt = ([0], [rows])
        self.first = np.ascontiguousarray(np.asarray(utt[0]), dtype=np.int64).reshape(-1)
        self.count = np.ascontiguousarray(np.asarray(utt[1]), dtype=np.int64).reshape(-1)
        if self.first.shape != self.count.shape or self.first.shape[0] < 1:
            raise ValueError(f"{what}: utt = (first, count), two arrays of one length, an utterance or more")
        self.n_utts = int(self.first.shape[0])
        self.n_total = int(np.maximum(self.count, 0).sum())
        ldx = feats.stride(0) if rows > 1 else max(feats.stride(0), D)
        self.struct = _hip.GmmFrames(feats.data_ptr(), _hip.GMM_X_F32 if feats.dtype == torch.float32 else _hip.GMM_X_F64, 0, rows, ldx,
                                     i64_ptr(self.first), i64_ptr(self.count), self.n_utts)
        self.device = feats.device

    def ref(self):
        return C.byref(self.struct)


def _options(reg_covar, var_floor, min_count):
    return _hip.GmmMstepOptions(float(reg_covar), float(var_floor), float(min_count))


@dataclass
class GmmStats:
    """Baum-Welch statistics of U utterances: n [U, C] (zeroth order), f [U, C, D] (first order, not centred), the sum of the
    frame log-likelihoods llsum [U] and the good frames n_frames [U] (int64); device tensors."""
    n: torch.Tensor
    f: torch.Tensor
    llsum: torch.Tensor = None
    n_frames: torch.Tensor = None
    n_bad: int = 0

    def stat_object(self, modelset, segset):
        """A plda.StatObject with stat0 [U, C] and stat1 [U, C D] in SIDEKIT's layout (component-major)."""
        from .plda import StatObject
        U = self.n.shape[0]
        return StatObject(modelset=modelset, segset=segset, stat1=self.f.reshape(U, -1).cpu().numpy(), stat0=self.n.cpu().numpy())


class DiagGmm:
    """A diagonal-covariance Gaussian mixture on the device: weights [C], means [C, D], variances [C, D], float64."""

    def __init__(self, weights, means, variances, device="cuda:0"):
        device = require_device(device, "DiagGmm")
        self.weights = dev_f64(weights, device).reshape(-1)
        self.means = dev_f64(means, device)
        self.variances = dev_f64(variances, device)
        C_, = self.weights.shape
        if self.means.dim() != 2 or self.means.shape[0] != C_ or self.variances.shape != self.means.shape:
            raise ValueError("DiagGmm: weights [C], means [C, D], variances [C, D]")
        if not (1 <= C_ <= MAX_C and 1 <= self.means.shape[1] <= MAX_D):
            raise ValueError(f"DiagGmm: C must lie in 1 .. {MAX_C}, D in 1 .. {MAX_D}")
        self.lower_bounds = None
        self.n_iter_ = 0
        self.n_bad = 0

    @property
    def device(self):
        return self.weights.device

    @property
    def n_components(self):
        return self.weights.shape[0]

    @property
    def dim(self):
        return self.means.shape[1]

    def to(self, device):
        return DiagGmm(self.weights, self.means, self.variances, device=device)

    def save(self, path):
        np.savez(path, weights=self.weights.cpu().numpy(), means=self.means.cpu().numpy(), variances=self.variances.cpu().numpy())

    @classmethod
    def load(cls, path, device="cuda:0"):
        with np.load(path) as z:
            return cls(z["weights"], z["means"], z["variances"], device=device)

    def prepared(self, means=None):
        """(P [C, 2D], g [C]): the prepared form of xvec_gmm_prepare, with `means` in place of the model's if given."""
        C_, D = self.n_components, self.dim
        P = torch.empty(C_, 2 * D, dtype=torch.float64, device=self.device)
        g = torch.empty(C_, dtype=torch.float64, device=self.device)
        mo = None if means is None else dev_f64(means, self.device)
        _check(_hip.lib.xvec_gmm_prepare(_p(self.weights), _p(self.means), _p(self.variances), _p(mo), C_, D, _p(P), _p(g),
                                         _stream(self.device)))
        return P, g

    def _loglik(self, feats, utt, means=None, posteriors=False):
        C_, D = self.n_components, self.dim
        fr = _Frames(feats, utt, D, "DiagGmm.log_likelihood")
        dev = fr.device
        need = _hip.lib.xvec_gmm_loglik_workspace_bytes(fr.n_utts, C_, D)
        ws = sized_workspace(need, lambda: ValueError("DiagGmm: too many utterances"), dev)
        lse = torch.empty(max(fr.n_total, 1), dtype=torch.float64, device=dev)
        llsum = torch.empty(fr.n_utts, dtype=torch.float64, device=dev)
        cnt = torch.empty(fr.n_utts, dtype=torch.int64, device=dev)
        n_bad = torch.empty(1, dtype=torch.int64, device=dev)
        gamma = torch.empty(max(fr.n_total, 1), C_, dtype=torch.float64, device=dev) if posteriors else None
        mo = None if means is None else dev_f64(means, dev)
        _check(_hip.lib.xvec_gmm_loglik(fr.ref(), _p(self.weights), _p(self.means), _p(self.variances), _p(mo), C_, D, _p(lse),
                                        _p(llsum), _p(cnt), _p(n_bad), _p(gamma), _p(ws), ws.numel(), _stream(dev)))
        torch.cuda.current_stream(dev).synchronize()       # the host arrays of `fr` were read in stream order
        return lse[:fr.n_total], llsum, cnt, n_bad, None if gamma is None else gamma[:fr.n_total]

    def log_likelihood(self, feats, utt=None, means=None):
        """(lse [n_total], llsum [U], n_frames [U]): the log-likelihood of every frame of the utterances, and per utterance
        the sum over, and the count of, its good frames.  `means` [C, D]: other means, e.g. a MAP-adapted model."""
        lse, llsum, cnt, _, _ = self._loglik(feats, utt, means)
        return lse, llsum, cnt

    def posteriors(self, feats, utt=None):
        """[n_total, C] dense posteriors (rows of zeros for bad frames): for small C and for tests."""
        return self._loglik(feats, utt, posteriors=True)[4]

    def _accumulate(self, feats, utt, per_utt, n_slices=0, workspace=None):
        C_, D = self.n_components, self.dim
        fr = _Frames(feats, utt, D, "DiagGmm.stats")
        dev = fr.device
        need = _hip.lib.xvec_gmm_accumulate_workspace_bytes(fr.n_total, fr.n_utts, C_, D, int(per_utt), int(n_slices))
        ws = sized_workspace(need, lambda: ValueError(f"DiagGmm: n_slices = {n_slices} must lie in 0 .. 1024 (0 per utterance)"), dev,
                             workspace)
        U = fr.n_utts if per_utt else 1
        n = torch.empty(U, C_, dtype=torch.float64, device=dev)
        f = torch.empty(U, C_, D, dtype=torch.float64, device=dev)
        s = None if per_utt else torch.empty(C_, D, dtype=torch.float64, device=dev)
        llsum = torch.empty(U, dtype=torch.float64, device=dev)
        cnt = torch.empty(U, dtype=torch.int64, device=dev)
        n_bad = torch.empty(1, dtype=torch.int64, device=dev)
        _check(_hip.lib.xvec_gmm_accumulate(fr.ref(), _p(self.weights), _p(self.means), _p(self.variances), C_, D, int(per_utt),
                                            int(n_slices), _p(n), _p(f), _p(s), _p(llsum), _p(cnt), _p(n_bad), _p(ws), ws.numel(),
                                            _stream(dev)))
        torch.cuda.current_stream(dev).synchronize()
        return n, f, s, llsum, cnt, n_bad

    def estep(self, feats, utt=None, n_slices=0, workspace=None):
        """The global statistics of one E-step: (n [C], f [C, D], s [C, D], llsum, n_frames, n_bad) as device tensors.
        `workspace`: a uint8 device tensor to use if it is large enough (what it holds does not matter)."""
        n, f, s, llsum, cnt, n_bad = self._accumulate(feats, utt, False, n_slices, workspace)
        return n[0], f[0], s, llsum, cnt, n_bad

    def stats(self, feats, utt=None, workspace=None) -> GmmStats:
        """The Baum-Welch statistics of every utterance."""
        n, f, _, llsum, cnt, n_bad = self._accumulate(feats, utt, True, 0, workspace)
        return GmmStats(n, f, llsum, cnt, int(n_bad.item()))

    def mstep(self, n, f, s, n_frames, reg_covar=1e-6, var_floor=0.0, min_count=0.0):
        """New weights, means and variances from the statistics of an E-step, in place."""
        opt = _options(reg_covar, var_floor, min_count)
        _check(_hip.lib.xvec_gmm_mstep(_p(n), _p(f), _p(s), _p(n_frames), self.n_components, self.dim, C.byref(opt), _p(self.weights),
                                       _p(self.means), _p(self.variances), _stream(self.device)))
        return self

    def em(self, feats, utt=None, n_iter=10, tol=0.0, reg_covar=1e-6, var_floor=0.0, min_count=0.0, n_slices=0):
        """Up to n_iter EM iterations in place, nothing read back in between; sets lower_bounds, n_iter_ and n_bad."""
        C_, D = self.n_components, self.dim
        fr = _Frames(feats, utt, D, "DiagGmm.em")
        if fr.n_total == 0:
            raise ValueError("DiagGmm.em: the utterances hold no frame")
        dev = fr.device
        need = _hip.lib.xvec_gmm_em_workspace_bytes(fr.n_total, fr.n_utts, C_, D, int(n_slices))
        ws = sized_workspace(need, lambda: ValueError(f"DiagGmm.em: n_slices = {n_slices} must lie in 0 .. 1024"), dev)
        lb = torch.empty(int(n_iter), dtype=torch.float64, device=dev)
        done = torch.empty(1, dtype=torch.int32, device=dev)
        n_bad = torch.empty(1, dtype=torch.int64, device=dev)
        opt = _options(reg_covar, var_floor, min_count)
        _check(_hip.lib.xvec_gmm_em(fr.ref(), C_, D, int(n_iter), float(tol), C.byref(opt), int(n_slices), _p(self.weights),
                                    _p(self.means), _p(self.variances), _p(lb), _p(done), _p(n_bad), _p(ws), ws.numel(), _stream(dev)))
        self.n_iter_ = int(done.item())
        self.lower_bounds = lb[:self.n_iter_].cpu().numpy()
        self.n_bad = int(n_bad.item())
        return self


def fit_ubm(feats, n_components, *, utt=None, n_iter=10, tol=1e-3, reg_covar=1e-6, init="frames", seed=0, var_floor=0.0,
            min_count=0.0, n_slices=0) -> DiagGmm:
    """Train a UBM by EM.  init="frames": `n_components` distinct frames of the utterances, drawn with `seed`, as the means,
    the global variance (+ reg_covar) for every component and uniform weights; or init = (weights, means, variances).
    tol is scikit-learn's: stop when the mean log-likelihood per frame moves by less than tol (0: run n_iter iterations)."""
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise RuntimeError("fit_ubm runs on a HIP device only (no CPU path): the features must be a device tensor")
    if feats.dim() == 3 and utt is None:
        feats, utt = frames_of(feats, [feats.shape[1]] * feats.shape[0])
    dev = feats.device
    if isinstance(init, str):
        if init != "frames":
            raise ValueError(f"init = {init!r}: 'frames' or (weights, means, variances)")
        D = feats.shape[1]
        fr = _Frames(feats, utt, D, "fit_ubm")
        rows = np.concatenate([np.arange(a, a + n) for a, n in zip(fr.first, fr.count)]) if fr.n_total else np.zeros(0, np.int64)
        rows = np.unique(rows)
        x = fr.x[torch.from_numpy(rows).to(dev)].to(torch.float64)
        finite = torch.isfinite(x).all(dim=1)
        x = x[finite]                                                      # a bad frame is neither a mean nor part of the variance
        if x.shape[0] < n_components:
            raise ValueError(f"fit_ubm: {n_components} components need as many distinct finite frames, got {x.shape[0]}")
        pick = np.sort(np.random.default_rng(seed).choice(x.shape[0], int(n_components), replace=False))
        means = x[torch.from_numpy(pick).to(dev)]
        var = x.var(dim=0, unbiased=False) + reg_covar
        init = (torch.full((int(n_components),), 1.0 / n_components, dtype=torch.float64), means, var.expand(int(n_components), D))
    gmm = DiagGmm(*init, device=dev)
    if gmm.n_components != n_components:
        raise ValueError(f"fit_ubm: init holds {gmm.n_components} components, not {n_components}")
    return gmm.em(feats, utt, n_iter=n_iter, tol=tol, reg_covar=reg_covar, var_floor=var_floor, min_count=min_count, n_slices=n_slices)


def _model_tensor(t, shape, dev, what):
    """`t` as the library reads it: a contiguous float64 tensor of `shape` (None: any length) on `dev`."""
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or t.dim() != len(shape) or \
            any(want is not None and have != want for have, want in zip(t.shape, shape)) or t.shape[0] < 1:
        want = ", ".join("*" if v is None else str(v) for v in shape)
        raise ValueError(f"{what}: expected a float64 tensor [{want}] on {dev}")
    return t.contiguous()


def map_adapt(ubm: DiagGmm, stats: GmmStats, relevance=16.0) -> torch.Tensor:
    """[M, C, D] relevance-MAP means of the M rows of `stats`; a component without frames keeps the UBM's mean exactly."""
    C_, D = ubm.n_components, ubm.dim
    n = _model_tensor(stats.n, (None, C_), ubm.device, "map_adapt: stats.n")
    f = _model_tensor(stats.f, (n.shape[0], C_, D), ubm.device, "map_adapt: stats.f")
    M = n.shape[0]
    out = torch.empty(M, C_, D, dtype=torch.float64, device=ubm.device)
    _check(_hip.lib.xvec_gmm_map_means(_p(n), _p(f), _p(ubm.means), M, C_, D, float(relevance), _p(out), _stream(ubm.device)))
    return out


def linear_scores(ubm: DiagGmm, model_means: torch.Tensor, test_stats: GmmStats) -> torch.Tensor:
    """[M, U] Glembek's linear scores of M models against U test utterances, float64 on the device in PldaScorer.score's
    layout: the first-order expansion of the average LLR per frame."""
    C_, D, dev = ubm.n_components, ubm.dim, ubm.device
    mm = _model_tensor(model_means, (None, C_, D), dev, "linear_scores: model_means")
    n = _model_tensor(test_stats.n, (None, C_), dev, "linear_scores: test_stats.n")
    f = _model_tensor(test_stats.f, (n.shape[0], C_, D), dev, "linear_scores: test_stats.f")
    M, U = mm.shape[0], n.shape[0]
    need = _hip.lib.xvec_gmm_linear_scores_workspace_bytes(M, U, C_, D)
    ws = sized_workspace(need, lambda: ValueError("linear_scores: a model and a test utterance or more"), dev)
    S = torch.empty(M, U, dtype=torch.float64, device=dev)
    _check(_hip.lib.xvec_gmm_linear_scores(_p(mm), M, _p(n), _p(f), U, _p(ubm.means), _p(ubm.variances), C_, D, _p(S), U, _p(ws),
                                           ws.numel(), _stream(dev)))
    return S


def llr_scores(ubm: DiagGmm, model_means: torch.Tensor, feats, utt=None) -> torch.Tensor:
    """[M, U] exact average log-likelihood ratio per good frame of each model against the UBM (NaN for an utterance without
    good frames): a host loop over the models around xvec_gmm_loglik."""
    _, base, cnt = ubm.log_likelihood(feats, utt)
    rows = [(ubm.log_likelihood(feats, utt, means=model_means[m])[1] - base) / cnt.to(torch.float64) for m in range(model_means.shape[0])]
    return torch.stack(rows)
