"""Embedding conditioning on the GPU: LDA, centring, whitening, length norm -- the step between the extractor and the PLDA
back end (include/xvec_lda.h).

The reference reduces x-vectors with speechbrain's `LDA().do_lda(stat, reduced_dim)` (plda_classifier.py:103-106, called on
every split at plda_score_stat.py:207-212); the recipe an x-vector back end normally runs is centre -> (whiten | LDA) ->
length-normalise -> PLDA.  Everything that grows with the number of vectors runs in HIP, in fp64 on the matrix pipe: ONE
statistics pass (mean, class means, the class-weighted within-class scatter and the between-class scatter) and ONE launch per
transform (centring, the product and the row norm together).  The D x D eigenproblem stays on the host in float64.

    new_stat = lda(x_vec_stat, reduced_dim=2)                  # drop-in for plda_classifier.lda

    tf = EmbeddingTransform.fit(train_xvecs, labels, lda_dim=150)      # centre -> LDA -> length norm: one launch per apply
    scores = scorer.score(tf.apply(enroll), tf.apply(test))            # device tensors throughout; nothing crosses to the host

    tf = EmbeddingTransform([EmbeddingTransform.center(mu), EmbeddingTransform.whiten(None, sigma),
                             EmbeddingTransform.length_norm()])

Parity with speechbrain itself is UNPINNED (not installed); tests/lda_ref.py restates its arithmetic in numpy float64 and the
tests check this module against it.  speechbrain takes `eig(inv(Sw) @ Sb)`; `lda_matrix_from_scatter` solves the same problem
as the symmetric-definite `eigh(Sb, Sw)`, scales every column to unit 2-norm and fixes its sign so that the component of
largest magnitude is positive (LAPACK's sign is arbitrary; this one is documented).  There is no CPU path.
"""
from __future__ import annotations

import copy
import sys
import types

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, dev_f64, i64_ptr, require_device, stream as _stream
from .plda import _labels

__all__ = ["lda_matrix_from_scatter", "embed_transform", "LdaStats", "LDA", "lda", "EmbeddingTransform", "NORM_CLIP"]

NORM_CLIP = 1e-8          # speechbrain's norm_stat1: a row is divided by max(its 2-norm, 1e-8)

_check = checker(_hip.lib.xvec_lda_last_error)


def lda_matrix_from_scatter(Sw, Sb, rank) -> np.ndarray:
    """[D, rank] float64: the eigenvectors of the `rank` largest eigenvalues of inv(Sw) Sb, largest first, each of unit
    2-norm with its largest-magnitude component positive.  Host only (scipy)."""
    from scipy import linalg
    Sw = np.asarray(Sw, dtype=np.float64)
    Sb = np.asarray(Sb, dtype=np.float64)
    if Sw.ndim != 2 or Sw.shape[0] != Sw.shape[1] or Sb.shape != Sw.shape:
        raise ValueError(f"lda_matrix_from_scatter: Sw and Sb must be square and alike, got {Sw.shape} and {Sb.shape}")
    dim = Sw.shape[0]
    if not 1 <= int(rank) <= dim:
        raise ValueError(f"rank = {rank} must lie in [1, dim = {dim}]")
    rank = int(rank)
    evals, evecs = linalg.eigh(0.5 * (Sb + Sb.T), 0.5 * (Sw + Sw.T))
    L = evecs[:, np.argsort(evals)[::-1][:rank]]
    L = L / np.linalg.norm(L, axis=0)
    cols = np.arange(rank)
    return L * np.sign(L[np.abs(L).argmax(0), cols])


def embed_transform(x, mean=None, w=None, normalize=False, device="cuda:0", out=None, workspace=None) -> torch.Tensor:
    """(x - mean) w on the device, float64, with every row divided by max(its norm, 1e-8) if `normalize`: one launch.
    `x` [N, D] device tensor (float32 / float64, unit column stride) or host array; `mean` [D] or None (no centring); `w`
    [D, R] or None (the identity: no product)."""
    device = require_device(device, "the embedding transform")
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64) \
            and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.device == device:
        t = x.detach()
    else:
        t = dev_f64(x, device, keep_f32=True)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"embed_transform: expected [N, D] vectors, got shape {tuple(t.shape)}")
    n, dim = int(t.shape[0]), int(t.shape[1])
    m = None if mean is None else dev_f64(mean, device)
    if m is not None and m.shape != (dim,):
        raise ValueError(f"embed_transform: mean of shape {tuple(m.shape)} for vectors of dimension {dim}")
    wd = None if w is None else dev_f64(w, device)
    if wd is not None and (wd.dim() != 2 or wd.shape[0] != dim):
        raise ValueError(f"embed_transform: w of shape {tuple(wd.shape)} for vectors of dimension {dim}")
    rank = dim if wd is None else int(wd.shape[1])
    if out is None:
        out = torch.empty((n, rank), dtype=torch.float64, device=device)
    elif (not isinstance(out, torch.Tensor) or out.device != device or out.dtype != torch.float64 or out.shape != (n, rank)
          or out.stride(1) != 1 or out.stride(0) < rank):
        raise ValueError("embed_transform: out must be a float64 device matrix [N, rank] with unit column stride")
    ws = byte_workspace(int(_hip.lib.xvec_embed_transform_workspace_bytes(n, dim, rank)), device, workspace)
    xd = _hip.LDA_X_F32 if t.dtype == torch.float32 else _hip.LDA_X_F64
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_embed_transform(t.data_ptr(), xd, n, dim, t.stride(0), None if m is None else m.data_ptr(),
                                             None if wd is None else wd.data_ptr(), rank, int(bool(normalize)),
                                             out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), _stream(device)))
    return out


class LdaStats:
    """The N-scale pass of LDA, run once on a HIP device: `mean` [D], `class_means` [C, D], `s_within` [D, D] (every class's
    biased covariance, summed), `s_between` [D, D] (exactly symmetric, both) and `classes` (sorted label names), numpy
    float64.  `matrix(rank)` solves the eigenproblem from them; several ranks share the pass."""

    def __init__(self, x, labels, device="cuda:0"):
        self.device = require_device(device, "LDA")
        t = dev_f64(x, self.device, keep_f32=True)
        if t.dim() != 2:
            raise ValueError(f"LdaStats: expected [N, D] x-vectors, got shape {tuple(t.shape)}")
        n, dim = int(t.shape[0]), int(t.shape[1])
        self.classes, order, start = _labels(labels, n)
        C = int(self.classes.shape[0])
        self.n, self.dim, self.n_classes = n, dim, C
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        mean, cm = torch.empty(dim, **f64), torch.empty((C, dim), **f64)
        sw, sb = torch.empty((dim, dim), **f64), torch.empty((dim, dim), **f64)
        order_d = torch.from_numpy(order).to(dev)
        ws = byte_workspace(_hip.lib.xvec_lda_stats_workspace_bytes(n, dim, C), dev)
        xd = _hip.LDA_X_F32 if t.dtype == torch.float32 else _hip.LDA_X_F64
        with torch.cuda.device(dev):
            _check(_hip.lib.xvec_lda_stats(t.data_ptr(), xd, n, dim, order_d.data_ptr(), i64_ptr(start), C, mean.data_ptr(),
                                           cm.data_ptr(), sw.data_ptr(), sb.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
        self.mean = mean.cpu().numpy()
        self.class_means = cm.cpu().numpy()
        self.s_within = sw.cpu().numpy()
        self.s_between = sb.cpu().numpy()

    def matrix(self, rank) -> np.ndarray:
        """[D, rank] LDA matrix (see lda_matrix_from_scatter).  Beyond C - 1 the eigenvalues are zero and the vectors
        arbitrary, so `rank` must lie in [1, min(D, C - 1)]."""
        top = min(self.dim, self.n_classes - 1)
        if not 1 <= int(rank) <= top:
            raise ValueError(f"rank = {rank} must lie in [1, min(dim, classes - 1) = {top}]")
        return lda_matrix_from_scatter(self.s_within, self.s_between, int(rank))


class LDA:
    """speechbrain.processing.PLDA_LDA.LDA's surface as the reference uses it: `do_lda` rotates a stat object's `stat1`
    by the LDA matrix of its own classes (or by `transform_mat`).  No centring, as speechbrain does none."""

    def __init__(self, device="cuda:0"):
        self.transform_mat = None
        self.device = str(device)

    def do_lda(self, stat_server=None, reduced_dim=2, transform_mat=None):
        if transform_mat is None:
            self.transform_mat = stat_server.get_lda_matrix_stat1(reduced_dim, device=self.device)
        else:
            self.transform_mat = np.asarray(transform_mat, dtype=np.float64)
        new_train_obj = copy.deepcopy(stat_server)
        new_train_obj.rotate_stat1(self.transform_mat, device=self.device)
        return new_train_obj


def lda(x_vec_stat, reduced_dim=2, device="cuda:0"):
    """plda_classifier.lda"""
    return LDA(device=device).do_lda(x_vec_stat, reduced_dim=reduced_dim)


def whitening_matrix(sigma) -> np.ndarray:
    """speechbrain's whiten_stat1 rotation: 2-D sigma -> V diag(1 / sqrt(lam)) with the eigenvalues descending; 1-D sigma
    (a diagonal covariance) -> diag(1 / sqrt(sigma)).  Host only."""
    from scipy import linalg
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim == 1:
        return np.diag(1.0 / np.sqrt(sigma))
    if sigma.ndim != 2 or sigma.shape[0] != sigma.shape[1]:
        raise ValueError(f"whiten: sigma must be [D] or [D, D], got {sigma.shape}")
    evals, evecs = linalg.eigh(sigma)
    ind = np.argsort(evals)[::-1]
    return evecs[:, ind] * (1.0 / np.sqrt(evals[ind]))[None, :]


class EmbeddingTransform:
    """A chain of conditioning stages, applied on the device.  Stages come from the static constructors `center(mu)`,
    `rotate(R)`, `whiten(mu, sigma)`, `lda(matrix)` and `length_norm()`.  Consecutive affine stages are composed on the
    host in float64 into one (mean, W) with y = (x - mean) W; every `length_norm` closes a launch, and so does a `center`
    that follows a rotation (it cannot be folded in front of one).  Centre -> LDA -> length norm is ONE launch.
    `launches` lists what runs: (mean or None, W or None, normalize).  Picklable: only host arrays are stored."""

    @staticmethod
    def center(mu):
        return ("center", np.asarray(mu, dtype=np.float64).copy())

    @staticmethod
    def rotate(R):
        R = np.asarray(R, dtype=np.float64)
        if R.ndim != 2:
            raise ValueError(f"rotate: a [D, R] matrix, got shape {R.shape}")
        return ("rotate", R.copy())

    @staticmethod
    def whiten(mu, sigma):
        """Centre by `mu` (None: no centring) and rotate by speechbrain's whitening matrix of `sigma`."""
        return ("whiten", None if mu is None else np.asarray(mu, dtype=np.float64).copy(), whitening_matrix(sigma))

    @staticmethod
    def lda(matrix):
        return EmbeddingTransform.rotate(matrix)

    @staticmethod
    def length_norm():
        return ("length_norm",)

    def __init__(self, stages, device="cuda:0"):
        self.device = str(device)
        self.launches = []
        mean, W = None, None

        def close(normalize):
            nonlocal mean, W
            if mean is not None or W is not None or normalize:
                self.launches.append((mean, W, normalize))
            mean, W = None, None

        for st in stages:
            kind = st[0]
            if kind not in ("center", "rotate", "whiten", "length_norm"):
                raise ValueError(f"EmbeddingTransform: unknown stage {kind!r}")
            if kind in ("center", "whiten") and st[1] is not None:
                if W is not None:
                    close(False)
                mean = st[1].copy() if mean is None else mean + st[1]
            if kind in ("rotate", "whiten"):
                R = st[-1]
                if W is not None and W.shape[1] != R.shape[0]:
                    raise ValueError(f"EmbeddingTransform: a rotation [{R.shape[0]}, ..] after one to {W.shape[1]} columns")
                W = R.copy() if W is None else W @ R
            if kind == "length_norm":
                close(True)
        close(False)
        for m, R, _ in self.launches:
            if R is not None and R.shape[1] > R.shape[0]:
                raise ValueError("EmbeddingTransform: a rotation must not add columns (rank <= dim)")
            if m is not None and R is not None and m.shape != (R.shape[0],):
                raise ValueError(f"EmbeddingTransform: mean {m.shape} in front of a rotation {R.shape}")
        self._dev = None

    def __getstate__(self):
        return {"device": self.device, "launches": self.launches}

    def __setstate__(self, state):
        self.device, self.launches, self._dev = state["device"], state["launches"], None

    def _device_launches(self):
        if self._dev is None:
            dev = require_device(self.device, "the embedding transform")
            up = lambda a: None if a is None else dev_f64(a, dev)
            self._dev = [(up(m), up(W), nrm) for m, W, nrm in self.launches]
        return self._dev

    def apply(self, x) -> torch.Tensor:
        """`x` [N, D] (device float32 / float64 tensor; a host array is uploaded) -> device float64 [N, R]."""
        dev = require_device(self.device, "the embedding transform")
        y = x
        for m, W, nrm in self._device_launches():
            y = embed_transform(y, m, W, nrm, device=dev)
        if y is x:                                    # no stage at all: still a device float64 tensor
            y = dev_f64(x, dev)
        return y

    @classmethod
    def fit(cls, x, labels, lda_dim=None, whiten=False, length_norm=True, device="cuda:0"):
        """The usual recipe from training vectors: centre by their mean, then whiten by their total covariance (`whiten`)
        and / or reduce to `lda_dim` dimensions by the LDA of `labels` (trained on the whitened vectors if both), then
        length-normalise (`length_norm`)."""
        dev = require_device(device, "the embedding transform")
        stages = []
        if whiten or lda_dim is None:
            from .plda import PldaStats
            st = PldaStats(x, labels, device=dev)
            stages.append(cls.whiten(st.mean, st.sigma_obs) if whiten else cls.center(st.mean))
        if lda_dim is not None:
            if whiten:
                st = LdaStats(cls(stages, device=dev).apply(x), labels, device=dev)
            else:
                st = LdaStats(x, labels, device=dev)
                stages.append(cls.center(st.mean))
            stages.append(cls.lda(st.matrix(lda_dim)))
        if length_norm:
            stages.append(cls.length_norm())
        return cls(stages, device=dev)


class _CallableModule(types.ModuleType):
    """`xvector_amd.lda` names both this module and the reference's function `lda`: the module is callable as that
    function, so `xvector_amd.lda(stat, 2)` and `xvector_amd.lda.LdaStats` both work."""

    def __call__(self, x_vec_stat, reduced_dim=2, device="cuda:0"):
        return lda(x_vec_stat, reduced_dim=reduced_dim, device=device)


sys.modules[__name__].__class__ = _CallableModule
