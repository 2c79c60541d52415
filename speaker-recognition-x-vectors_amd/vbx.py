"""VBx on the GPU: diarization's refinement step behind the clustering (include/xvec_vbx.h).

AHC labels every window on its own from pairwise scores; VBx (Landini et al.) is a Bayesian HMM whose states are speakers, with
PLDA-shaped speaker priors and a loop probability that models turn-taking.  Variational Bayes re-assigns the windows from the
order they come in and from speaker models estimated over all of a speaker's windows, and drops redundant speakers.  The
kernels are checked against tests/vbx_ref.py, a numpy restatement of the header's specification; the VBx package is not a
dependency and parity with it is unpinned.

    vm = VbxModel.from_plda(plda)                               # host, model-sized: the projection and phi
    y = vm.project(window_xvecs)                                # [N, R] float64 on the device (embed_transform)
    res = vbx(y, rec_start, vm.phi, init_labels=cl.labels, n_speakers=10)
    res.labels, res.n_speakers, res.gamma, res.pi, res.elbo, res.iters      # device tensors

    d = Diarizer(model, scorer, transform, threshold=0.0, resegment=Vbx(vm, n_speakers=10))

There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, dev_f64, i64_ptr, rec_start as _dev_rec_start, require_device, stream as _stream

__all__ = ["vbx", "vbx_init", "Vbx", "VbxModel", "VbxResult", "MAX_SPEAKERS", "MAX_DIM", "MAX_FRAMES", "THREADS", "PREFETCH"]

# include/xvec_vbx.h: the most speakers, dimensions and frames of a recording, the threads of a recording's block, the frames
# the recurrence loads ahead
MAX_SPEAKERS, MAX_DIM, MAX_FRAMES, THREADS, PREFETCH = 64, 512, 16384, 256, 8

_check = checker(_hip.lib.xvec_vbx_last_error)


class VbxResult(NamedTuple):
    gamma: torch.Tensor           # [N, S] float64: the responsibilities
    pi: torch.Tensor              # [n_rec, S] float64: the speaker priors
    elbo: torch.Tensor            # [n_rec, max_iter] float64, NaN in the slots of iterations not run
    iters: torch.Tensor           # [n_rec] int32
    labels: torch.Tensor          # [N] int32: the speaker of every frame, numbered per recording in order of appearance
    n_speakers: torch.Tensor      # [n_rec] int32


class VbxModel:
    """The projection VBx works in: `A` [R, D] with A Sigma A^T = I and A F F^T A^T = diag(phi), `phi` [R] > 0 (largest
    first) and the PLDA mean.  Host side and model-sized; `project` runs on the device."""

    def __init__(self, mean, A, phi):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.phi = np.ascontiguousarray(phi, dtype=np.float64)
        if self.A.ndim != 2 or self.A.shape != (self.phi.shape[0], self.mean.shape[0]) or not (self.phi > 0).all():
            raise ValueError("VbxModel: A must be [R, D] with a positive phi [R] and a mean [D]")

    @classmethod
    def from_plda(cls, mean, F=None, Sigma=None, tol=1e-10):
        """From a PLDA model x = mean + F y + e, e ~ N(0, Sigma): `mean` [D], `F` [D, rank_f] and `Sigma` [D, D], or one object
        that carries the three (plda.PLDA).  Solves the generalised eigenproblem of F F^T against Sigma and keeps the
        directions whose eigenvalue is above tol times the largest (at most rank_f of them)."""
        from scipy import linalg
        if F is None and Sigma is None and hasattr(mean, "F"):
            mean, F, Sigma = mean.mean, mean.F, mean.Sigma
        mean = np.asarray(mean, dtype=np.float64).reshape(-1)
        F = np.asarray(F, dtype=np.float64)
        Sigma = np.asarray(Sigma, dtype=np.float64)
        dim = mean.shape[0]
        if F.ndim != 2 or F.shape[0] != dim or Sigma.shape != (dim, dim):
            raise ValueError(f"VbxModel.from_plda: mean [D], F [D, rank_f] and Sigma [D, D] expected, got {mean.shape}, {F.shape}, {Sigma.shape}")
        between = F @ F.T
        evals, evecs = linalg.eigh(0.5 * (between + between.T), 0.5 * (Sigma + Sigma.T))      # evecs^T Sigma evecs = I
        order = np.argsort(evals)[::-1][:F.shape[1]]
        order = order[evals[order] > tol * evals[order[0]]]
        if not len(order):
            raise ValueError("VbxModel.from_plda: F F^T has no positive direction")
        return cls(mean, evecs[:, order].T, evals[order])

    def project(self, x, device="cuda:0", workspace=None) -> torch.Tensor:
        """(x - mean) A^T, float64 [N, R] on the device."""
        from .lda import embed_transform
        return embed_transform(x, self.mean, self.A.T, device=device, workspace=workspace)


class Vbx(NamedTuple):
    """What `Diarizer(resegment=...)` runs behind the clustering: the model and the options of `vbx`."""
    model: VbxModel
    n_speakers: int = 10
    loop_prob: float = 0.99
    Fa: float = 0.3
    Fb: float = 17.0
    max_iter: int = 40
    epsilon: float = 1e-4
    init_smoothing: float = 5.0


def _frames(x, what) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): the x-vectors must be a device tensor")
    if x.dim() != 2 or x.dtype != torch.float64 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: expected float64 [N, D] x-vectors")
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def _rec_start(rec_start, n, what) -> np.ndarray:
    return _dev_rec_start(rec_start, n, what, "frames", "frame")


def vbx_init(labels, rec_start, n_speakers, smoothing=5.0):
    """(gamma [N, S], pi [n_rec, S]) float64 on the labels' device: softmax(smoothing * onehot(label)) per frame (a label
    outside 0 .. S - 1 gives a uniform row) and uniform priors."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("vbx_init runs on a HIP device only (no CPU path): the labels must be a device tensor")
    lab = labels.to(torch.int32).contiguous()
    rs = _rec_start(rec_start, int(lab.shape[0]), "vbx_init")
    n_rec, S, dev = rs.shape[0] - 1, int(n_speakers), lab.device
    gamma = torch.empty((lab.shape[0], max(S, 1)), dtype=torch.float64, device=dev)
    pi = torch.empty((n_rec, max(S, 1)), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(_hip.lib.xvec_vbx_init(lab.data_ptr(), i64_ptr(rs), n_rec, S, float(smoothing), gamma.data_ptr(),
                                      gamma.stride(0), pi.data_ptr(), _stream(dev)))
    return gamma, pi


def vbx(x, rec_start, phi, init_labels=None, gamma=None, pi=None, n_speakers=None, loop_prob=0.99, Fa=0.3, Fb=17.0, max_iter=40,
        epsilon=1e-4, init_smoothing=5.0, workspace=None) -> VbxResult:
    """VBx over the recordings of the device x-vectors x [N, D] (float64, already projected: VbxModel.project), recording r
    being rows rec_start[r] .. rec_start[r + 1] - 1 (host integers), with phi [D].  Start from `init_labels` [N] (the
    clustering's, with `n_speakers` HMM states) or from responsibilities `gamma` [N, S] (and priors `pi` [n_rec, S], uniform
    if left out); neither is modified.  One launch for all recordings and iterations."""
    xd = _frames(x, "vbx")
    dev = xd.device
    n, dim = int(xd.shape[0]), int(xd.shape[1])
    rs = _rec_start(rec_start, n, "vbx")
    n_rec = rs.shape[0] - 1
    ph = dev_f64(phi, dev)
    if ph.shape != (dim,):
        raise ValueError(f"vbx: phi of shape {tuple(ph.shape)} for x-vectors of dimension {dim}")
    if (init_labels is None) == (gamma is None):
        raise ValueError("vbx: give init_labels or gamma, one of the two")
    if gamma is None:
        if n_speakers is None:
            raise ValueError("vbx: init_labels need n_speakers, the number of HMM states")
        lab = init_labels if isinstance(init_labels, torch.Tensor) else torch.as_tensor(np.asarray(init_labels))
        if lab.shape != (n,):
            raise ValueError(f"vbx: {tuple(lab.shape)} labels for {n} frames")
        g, p = vbx_init(lab.to(dev), rs, int(n_speakers), init_smoothing)
    else:
        g = dev_f64(gamma, dev).clone()
        if g.dim() != 2 or g.shape[0] != n or (n_speakers is not None and g.shape[1] != int(n_speakers)):
            raise ValueError(f"vbx: gamma of shape {tuple(g.shape)} for {n} frames and n_speakers = {n_speakers}")
        S = int(g.shape[1])
        p = torch.full((n_rec, S), 1.0 / S, dtype=torch.float64, device=dev) if pi is None else dev_f64(pi, dev).clone()
        if p.shape != (n_rec, S):
            raise ValueError(f"vbx: pi of shape {tuple(p.shape)} for {n_rec} recordings of {S} speakers")
    S = int(g.shape[1])
    opts = _hip.VbxOptions(float(loop_prob), float(Fa), float(Fb), float(epsilon), int(max_iter), 0)
    rs_p = i64_ptr(rs)
    elbo = torch.empty((n_rec, max(int(max_iter), 1)), dtype=torch.float64, device=dev)
    iters = torch.empty(n_rec, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(n_rec, dtype=torch.int32, device=dev)
    ws = byte_workspace(int(_hip.lib.xvec_vbx_workspace_bytes(rs_p, n_rec, dim, S)), dev, workspace)
    with torch.cuda.device(dev):
        _check(_hip.lib.xvec_vbx_run(xd.data_ptr(), xd.stride(0), dim, ph.data_ptr(), rs_p, n_rec, S, _hip.C.byref(opts),
                                     g.data_ptr(), g.stride(0), p.data_ptr(), elbo.data_ptr(), iters.data_ptr(), labels.data_ptr(),
                                     count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return VbxResult(g, p, elbo, iters, labels, count)


def workspace_bytes(rec_start, dim, n_speakers) -> int:
    """Bytes of workspace `vbx` needs for these recordings (0: the arguments are refused)."""
    rs = np.ascontiguousarray(np.asarray(rec_start), dtype=np.int64)
    return int(_hip.lib.xvec_vbx_workspace_bytes(i64_ptr(rs), rs.shape[0] - 1, int(dim), int(n_speakers)))


def resegment(opts: Vbx, vecs, rec_start, labels, device, workspace=None) -> VbxResult:
    """What the Diarizer runs per call: the call's conditioned x-vectors through the model's projection, VBx from the
    clustering's labels."""
    y = opts.model.project(vecs, device=device)
    return vbx(y, rec_start, opts.model.phi, init_labels=labels, n_speakers=opts.n_speakers, loop_prob=opts.loop_prob, Fa=opts.Fa,
               Fb=opts.Fb, max_iter=opts.max_iter, epsilon=opts.epsilon, init_smoothing=opts.init_smoothing, workspace=workspace)
