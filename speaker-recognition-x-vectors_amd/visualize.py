"""Embedding maps on the GPU: what the reference's `plot_images` computes for its scatter plots -- a 2-D LDA, a 2-D PCA of the
standardised x-vectors and a 2-D t-SNE (plda_score_stat.py:207-224) -- without the plotting (include/xvec_tsne.h).

    maps = scatter_maps(checked_xvec, checked_label)           # {"LDA", "PCA", "TSNE"}: [N, 2] float64 device tensors
    y = tsne_map(xvecs, perplexity=30.0)                       # TSNE(2, method="exact").fit_transform(xvecs)
    z = pca_map(xvecs)                                         # PCA(2).fit_transform(StandardScaler().fit_transform(xvecs))

The reference calls `TSNE(2)`, scikit-learn's Barnes-Hut approximation.  Here the EXACT method runs (scikit-learn 1.7's
method='exact': the same perplexity search, gradient, gains and schedule): on the device it is an N^2 pass per iteration over a
matrix that stays in HBM, and needs no approximation.  All of it is fp64 HIP: squared distances (the Gram product on the fp64
matrix pipe), the perplexity search, and two launches per iteration.  The host reads back two numbers every 50 iterations (the
KL divergence and the gradient norm) for scikit-learn's stop rules; nothing else crosses before the final [N, 2] array is asked
for.  PCA takes the mean and the total scatter from the library's statistics pass, solves the D x D eigenproblem on the host as
lda.py does, and projects in one xvec_embed_transform launch.  There is no CPU path.

Parity: tests/tsne_ref.py restates the arithmetic in numpy; tests/golden/g11_tsne.npz pins it to scikit-learn 1.7.2 itself.  An
embedding cannot be compared point by point after more than a few iterations (t-SNE's descent amplifies a 1e-13 change of the
start to 1e-2 within 50), so whole runs are compared by KL divergence, trustworthiness and 1-NN label accuracy.  Two deviations
from scikit-learn, both documented in xvec_tsne.h: the gradient does not floor Q at eps, and the gradient norm of the
`min_grad_norm` stop is taken before the gains are applied.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, dev_f64, require_device, sized_workspace, stream as _stream

__all__ = ["pca_matrix_from_scatter", "pca_map", "squared_distances", "tsne_affinities", "tsne_plan", "Tsne", "tsne_map", "scatter_maps",
           "MAX_POINTS"]

MAX_POINTS = 8192                     # XVEC_TSNE_MAX_POINTS
_EXPLORATION = 250                    # TSNE._EXPLORATION_MAX_ITER
_CHECK = 50                           # TSNE._N_ITER_CHECK

_check = checker(_hip.lib.xvec_tsne_last_error)


def _vectors(x, device, what):
    """[N, D] float32 / float64 device tensor with unit column stride (a host array is uploaded)."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64) \
            and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.device == device:
        t = x.detach()
    else:
        t = dev_f64(x, device, keep_f32=True)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected [N, D] vectors, got shape {tuple(t.shape)}")
    return t


def _matrix(a, device, n, cols, what):
    """A float64 device matrix [n, cols] with unit column stride, as it is (strided views are passed on with their stride)."""
    if not (isinstance(a, torch.Tensor) and a.device == device and a.dtype == torch.float64 and tuple(a.shape) == (n, cols)
            and a.stride(1) == 1 and a.stride(0) >= cols):
        raise ValueError(f"{what} must be a float64 device matrix [{n}, {cols}] with unit column stride")
    return a


# ---------------------------------------------------------------- PCA

def pca_matrix_from_scatter(mean, cov, n, n_components=2, standardize=True) -> np.ndarray:
    """[D, n_components] float64 W with scores = (x - mean) W.  `cov` is the biased covariance of `n` vectors.  With
    `standardize` the columns are first divided by sqrt(diag cov) (1 for a constant column, by StandardScaler's test
    var <= n eps var + (n mean eps)^2) and the scaling is folded into W.  The components are the eigenvectors of the largest
    eigenvalues, largest first, each with its largest-magnitude entry positive (scikit-learn 1.7's
    svd_flip(u_based_decision=False)).  Host only."""
    cov = np.asarray(cov, dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    dim = cov.shape[0]
    if cov.shape != (dim, dim) or mean.shape != (dim,):
        raise ValueError(f"pca_matrix_from_scatter: mean {mean.shape} and covariance {cov.shape} do not belong together")
    if not 1 <= int(n_components) <= min(dim, int(n)):
        raise ValueError(f"n_components = {n_components} must lie in [1, min(dim, N) = {min(dim, int(n))}]")
    scale = np.ones(dim)
    if standardize:
        var = np.diag(cov).copy()
        eps = np.finfo(np.float64).eps
        constant = var <= n * eps * var + (n * mean * eps) ** 2
        scale = np.sqrt(var)
        scale[constant] = 1.0
    c = 0.5 * (cov + cov.T) / scale[:, None] / scale[None, :]
    lam, vec = np.linalg.eigh(c)
    vec = vec[:, np.argsort(lam)[::-1][:int(n_components)]]
    vec = vec * np.sign(vec[np.abs(vec).argmax(0), np.arange(vec.shape[1])])
    return vec / scale[:, None]


def pca_map(x, n_components=2, standardize=True, device="cuda:0") -> torch.Tensor:
    """[N, n_components] float64 on the device.  With `standardize` it is what the reference plots:
    PCA(n_components).fit_transform(StandardScaler().fit_transform(x)); without, PCA(n_components).fit_transform(x)."""
    from .lda import embed_transform
    from .plda import PldaStats
    device = require_device(device, "the PCA map")
    t = _vectors(x, device, "pca_map")
    n = int(t.shape[0])
    if n < 2:
        raise ValueError("pca_map: need at least two vectors")
    st = PldaStats(t, np.zeros(n, dtype=np.int64), device=device)      # one class: the mean and the total covariance
    w = pca_matrix_from_scatter(st.mean, st.sigma_obs, n, n_components, standardize)
    return embed_transform(t, st.mean, w, False, device=device)


# ---------------------------------------------------------------- t-SNE

def tsne_plan(n, cus=0) -> tuple:
    """(rows of a block, column slices, columns of a slice) of the pair pass for n points on `cus` compute units (0: the
    current device's).  Test introspection."""
    r, s, c = (_hip.C.c_int32(), _hip.C.c_int32(), _hip.C.c_int32())
    _check(_hip.lib.xvec_tsne_plan(int(n), int(cus), _hip.C.byref(r), _hip.C.byref(s), _hip.C.byref(c)))
    return r.value, s.value, c.value


def _workspace(n, d, device, cached=None):
    refusal = lambda: ValueError(f"t-SNE: n = {n} points must lie in 2 .. {MAX_POINTS} (and d = {d} in 0 .. 65536)")
    return sized_workspace(_hip.lib.xvec_tsne_workspace_bytes(int(n), int(d)), refusal, device, cached)


def squared_distances(x, round_distances=True, device="cuda:0", out=None, workspace=None) -> torch.Tensor:
    """[N, N] float64 squared Euclidean distances of the rows of `x`, scikit-learn's euclidean_distances(squared=True);
    with `round_distances` rounded to float32 and back, as scikit-learn's t-SNE does before its perplexity search."""
    device = require_device(device, "t-SNE")
    t = _vectors(x, device, "squared_distances")
    n, d = int(t.shape[0]), int(t.shape[1])
    ws = _workspace(n, d, device, workspace)
    out = torch.empty((n, n), dtype=torch.float64, device=device) if out is None else _matrix(out, device, n, n, "squared_distances: out")
    xd = _hip.TSNE_X_F32 if t.dtype == torch.float32 else _hip.TSNE_X_F64
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_tsne_sqdist(t.data_ptr(), xd, n, d, t.stride(0), int(bool(round_distances)), out.data_ptr(),
                                         out.stride(0), ws.data_ptr(), ws.numel(), _stream(device)))
    return out


def tsne_affinities(x=None, sqdist=None, perplexity=30.0, round_distances=True, device="cuda:0", out=None, betas=None,
                    workspace=None) -> torch.Tensor:
    """The dense symmetric joint probabilities P [N, N] (float64, on the device) of scikit-learn's _joint_probabilities, from
    the vectors `x` or from squared distances `sqdist` [N, N] (float64 device matrix; `round_distances` does not apply then).
    `betas` (optional float64 device vector [N]) receives every row's precision."""
    device = require_device(device, "t-SNE")
    if (x is None) == (sqdist is None):
        raise ValueError("tsne_affinities: pass the vectors x or the squared distances sqdist, one of them")
    if sqdist is None:
        sqdist = squared_distances(x, round_distances, device, workspace=workspace)
    elif not isinstance(sqdist, torch.Tensor):
        sqdist = dev_f64(sqdist, device)
    n = int(sqdist.shape[0])
    d2 = _matrix(sqdist, device, n, n, "tsne_affinities: sqdist")
    ws = _workspace(n, 0, device, workspace)
    out = torch.empty((n, n), dtype=torch.float64, device=device) if out is None else _matrix(out, device, n, n, "tsne_affinities: out")
    if betas is not None and not (isinstance(betas, torch.Tensor) and betas.device == device and betas.dtype == torch.float64
                                  and tuple(betas.shape) == (n,) and betas.is_contiguous()):
        raise ValueError(f"tsne_affinities: betas must be a contiguous float64 device vector [{n}]")
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_tsne_affinities(d2.data_ptr(), d2.stride(0), n, float(perplexity), out.data_ptr(), out.stride(0),
                                             None if betas is None else betas.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _stream(device)))
    return out


def run_schedule(step, n, max_iter=1000, early_exaggeration=12.0, learning_rate="auto", n_iter_without_progress=300,
                 min_grad_norm=1e-7):
    """scikit-learn's schedule for method='exact' (TSNE._tsne over _gradient_descent) on `step(count, exaggeration, momentum,
    learning_rate, fresh) -> (kl, grad_norm)`, which advances `count` iterations and reports the last one's KL divergence and
    gradient norm; `fresh` asks for a zero update and unit gains first, as each of scikit-learn's two descents starts.
    250 iterations at `early_exaggeration` and momentum 0.5, then momentum 0.8 up to `max_iter`; every 50th iteration is
    a check: the run stops when the KL divergence has not improved for more than 250 (first stage) / `n_iter_without_progress`
    iterations, or when the gradient norm is at most `min_grad_norm`; a stop in the first stage only opens the second.
    Returns (kl_divergence_, n_iter_: the index of the last iteration run)."""
    if max_iter < _EXPLORATION:
        raise ValueError(f"max_iter = {max_iter} must be at least {_EXPLORATION}")
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)

    def descent(it, last, patience, exaggeration, momentum):
        kl, best, best_iter, i = np.finfo(float).max, np.finfo(float).max, it, it
        while i < last:
            stop = min(last, (i // _CHECK + 1) * _CHECK)      # one past the next check iteration, or past the last one
            kl, norm = step(stop - i, exaggeration, momentum, lr, i == it)
            i = stop
            if stop % _CHECK == 0:
                if kl < best:
                    best, best_iter = kl, stop - 1
                elif stop - 1 - best_iter > patience:
                    break
                if norm <= min_grad_norm:
                    break
        return kl, max(i - 1, it)

    _, it = descent(0, _EXPLORATION, _EXPLORATION, float(early_exaggeration), 0.5)
    return descent(it + 1, int(max_iter), int(n_iter_without_progress), 1.0, 0.8)


class Tsne:
    """Exact t-SNE to two dimensions on a HIP device, scikit-learn's TSNE(2, method='exact') by its parameters.

        t = Tsne(x, perplexity=30.0, init="pca")         # distances, P and the start; nothing has moved yet
        t.step(50)                                       # 50 iterations at the current exaggeration / momentum
        y = t.run()                                      # or: the whole schedule; y is t.embedding_ ([N, 2], device)

    Holds P, Y, the update and the gains on the device with the workspace and the iteration count `n_iter`.  `init` is "pca"
    (pca_map(x, 2, standardize=False) scaled to a first column of standard deviation 1e-4), "random" (1e-4 times a normal
    draw from a host torch.Generator seeded with `seed`) or an [N, 2] array.  Either `x` or `P` (a dense joint matrix on the
    device, e.g. of tsne_affinities) must be given; init="pca" needs x."""

    def __init__(self, x=None, P=None, perplexity=30.0, init="pca", seed=0, early_exaggeration=12.0, learning_rate="auto",
                 max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, min_gain=0.01, round_distances=True,
                 device="cuda:0"):
        self.device = dev = require_device(device, "t-SNE")
        if (x is None) == (P is None):
            raise ValueError("Tsne: pass the vectors x or the joint probabilities P, one of them")
        xt = None if x is None else _vectors(x, dev, "Tsne")
        n = int(xt.shape[0] if P is None else P.shape[0])
        self.n = n
        self._ws = _workspace(n, 0 if xt is None else int(xt.shape[1]), dev)
        self.P = tsne_affinities(xt, None, perplexity, round_distances, dev, workspace=self._ws) if P is None \
            else _matrix(P, dev, n, n, "Tsne: P")
        if isinstance(init, str):
            if init == "pca":
                if xt is None:
                    raise ValueError("Tsne: init='pca' needs the vectors x")
                y = pca_map(xt, 2, standardize=False, device=dev)
                y = y * (1e-4 / y[:, 0].std(correction=0))
            elif init == "random":
                g = torch.Generator(device="cpu").manual_seed(int(seed))
                y = (1e-4 * torch.randn((n, 2), generator=g, dtype=torch.float64)).to(dev)
            else:
                raise ValueError(f"Tsne: init = {init!r} must be 'pca', 'random' or an [N, 2] array")
        else:
            y = dev_f64(init, dev).clone()
        if tuple(y.shape) != (n, 2):
            raise ValueError(f"Tsne: init of shape {tuple(y.shape)} for {n} points")
        self.Y = y.contiguous()
        self.update = torch.zeros_like(self.Y)
        self.gains = torch.ones_like(self.Y)
        self._report = torch.zeros(2, dtype=torch.float64, device=dev)      # KL, gradient norm
        self.early_exaggeration, self.learning_rate = float(early_exaggeration), learning_rate
        self.max_iter, self.n_iter_without_progress = int(max_iter), int(n_iter_without_progress)
        self.min_grad_norm, self.min_gain = float(min_grad_norm), float(min_gain)
        self.n_iter = 0
        self.embedding_, self.kl_divergence_, self.n_iter_ = None, None, None

    @property
    def learning_rate_(self) -> float:
        if self.learning_rate == "auto":
            return max(self.n / self.early_exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    def step(self, count=1, exaggeration=None, momentum=None, learning_rate=None, report=False, fresh=False):
        """`count` iterations.  Without `exaggeration` and `momentum` it follows scikit-learn's schedule by `n_iter`: 12 and 0.5
        before iteration 250, then 1 and 0.8 from a zero update and unit gains (a count that crosses 250 is split there).  With
        them, these values; `fresh` then asks for the zero update and unit gains.  With `report` returns (KL divergence of the Y
        that entered the last iteration, 2-norm of its gradient) -- one small read-back; without, nothing crosses and the call
        does not wait."""
        count = int(count)
        if exaggeration is None and momentum is None:
            early = self.n_iter < _EXPLORATION
            if early and self.n_iter + count > _EXPLORATION:
                first = _EXPLORATION - self.n_iter
                self.step(first, learning_rate=learning_rate, fresh=fresh)
                return self.step(count - first, learning_rate=learning_rate, report=report)
            exaggeration, momentum = (self.early_exaggeration, 0.5) if early else (1.0, 0.8)
            fresh = fresh or self.n_iter == _EXPLORATION
        elif exaggeration is None or momentum is None:
            raise ValueError("Tsne.step: pass both exaggeration and momentum, or neither")
        lr = self.learning_rate_ if learning_rate is None else float(learning_rate)
        if fresh:
            self.update.zero_()
            self.gains.fill_(1.0)
        rep = self._report
        with torch.cuda.device(self.device):
            _check(_hip.lib.xvec_tsne_steps(self.P.data_ptr(), self.P.stride(0), self.n, 2, self.Y.data_ptr(),
                                            self.update.data_ptr(), self.gains.data_ptr(), self.Y.stride(0), count,
                                            float(exaggeration), float(momentum), lr, self.min_gain,
                                            rep.data_ptr() if report else None, rep.data_ptr() + 8 if report else None,
                                            self._ws.data_ptr(), self._ws.numel(), _stream(self.device)))
        self.n_iter += count
        if report:
            kl, norm = rep.cpu().tolist()
            return kl, norm
        return None

    def run(self) -> torch.Tensor:
        """The whole schedule from iteration 0 (run_schedule); sets and returns `embedding_`, with `kl_divergence_` and
        `n_iter_` as scikit-learn reports them."""
        if self.n_iter != 0:
            raise RuntimeError("Tsne.run: the optimisation has already been advanced; make a new Tsne")

        def advance(count, exaggeration, momentum, lr, fresh):
            return self.step(count, exaggeration, momentum, lr, report=True, fresh=fresh)

        self.kl_divergence_, self.n_iter_ = run_schedule(advance, self.n, self.max_iter, self.early_exaggeration,
                                                         self.learning_rate, self.n_iter_without_progress, self.min_grad_norm)
        self.embedding_ = self.Y
        return self.Y


def tsne_map(x, **kw) -> torch.Tensor:
    """TSNE(2, method='exact', **kw).fit_transform(x): [N, 2] float64 on the device (the keywords are Tsne's)."""
    return Tsne(x, **kw).run()


def scatter_maps(x, labels, perplexity=30.0, device="cuda:0", **tsne_kw) -> dict:
    """One iteration of the loop at the end of the reference's plot_images, without the plotting: {"LDA", "PCA", "TSNE"} ->
    [N, 2] float64 device tensors of the x-vectors `x` [N, D] with speaker labels `labels` [N]."""
    from .lda import embed_transform
    from .plda import get_x_vec_stat
    device = require_device(device, "the embedding maps")
    t = _vectors(x, device, "scatter_maps")
    stat = get_x_vec_stat(t, labels)
    w = stat.get_lda_matrix_stat1(2, device=str(device))           # what lda.lda(stat, 2) rotates by
    return {"LDA": embed_transform(t, None, w, False, device=device),
            "PCA": pca_map(t, 2, standardize=True, device=device),
            "TSNE": tsne_map(t, perplexity=perplexity, device=device, **tsne_kw)}
