"""PLDA training on the GPU: the stage in front of the scorer (reference main.py:271-310).

The reference trains with speechbrain's `PLDA.plda(stat)` (plda_classifier.py:51-57) in numpy float64: the default
two-covariance EM with a low-rank between-class matrix F and a full residual covariance Sigma.  Here everything that grows
with the number of training vectors runs in HIP (include/xvec_plda.h): ONE statistics pass (mean, class counts, centred
class sums, the centred scatter matrix on fp64 MFMA) and, per EM iteration, the class-scale products.  The model-sized
factorizations stay on the host in float64, as `scoring.plda_constants` does.

    stats = PldaStats(x_vecs, labels)                 # x_vecs: [N, D] device tensor (fp32 / fp64) or numpy array
    mean, F, Sigma = stats.fit(rank_f=150)            # numpy float64; several ranks from one PldaStats
    plda = train_plda(setup_plda(rank_f=150), tr_stat) # drop-in for plda_classifier.setup_plda / train_plda

Each iteration is speechbrain's loop rewritten exactly (in exact arithmetic): with P = Sigma^-1 F (Cholesky solve),
A = F' P = Q diag(lam) Q', Y = S~ P Q (S~ the scaled centred class sums) and H = Y / (n lam + 1),
    sum_c E[hh'] = Q (diag(sum_c g_c) + H'H) Q',   _A = Q (diag(sum_c n_c g_c) + H' diag(n) H) Q',   _C = Q H' S~
(g_ck = 1 / (n_c lam_k + 1)): no whitening, no per-class R x R matrix, no D x D eigendecomposition per iteration.
Parity with speechbrain itself is UNPINNED (not installed); tests/plda_em_ref.py restates its loop literally and the tests
check this module against it.
"""
from __future__ import annotations

import pickle
import time

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, dev_f64, i64_ptr, require_device, stream as _stream

_check = checker(_hip.lib.xvec_plda_last_error)


def host_em(sigma_obs, counts, rank_f, nb_iter, products):
    """The EM loop's host half: returns (F, Sigma), numpy float64.  `sigma_obs` [D, D] and `counts` [C] (scaled) are the
    statistics, `products(pq, lam)` returns (H'H, H' diag(n) H, H' S~) of the iteration (R x R, R x R, R x D) for
    pq = Sigma^-1 F Q [D, R] and the eigenvalues lam of F' Sigma^-1 F -- `PldaStats` computes them on the device."""
    from scipy import linalg
    sigma_obs = np.asarray(sigma_obs, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    dim = sigma_obs.shape[0]
    if not 1 <= rank_f <= dim:
        raise ValueError(f"rank_f = {rank_f} must lie in [1, dim = {dim}]")
    evals, evecs = linalg.eigh(sigma_obs)
    F = evecs[:, np.argsort(evals)[::-1][:rank_f]]
    Sigma = sigma_obs.copy()
    n_classes, n_total = counts.shape[0], counts.sum()
    for _ in range(nb_iter):
        P = linalg.cho_solve(linalg.cho_factor(Sigma, lower=True), F)
        A = F.T @ P
        lam, Q = linalg.eigh(0.5 * (A + A.T))
        hh, nhh, hs = products(P @ Q, lam)
        g = 1.0 / (counts[:, None] * lam[None, :] + 1.0)
        e_hh = Q @ (np.diag(g.sum(0)) + hh) @ Q.T
        _A = Q @ (np.diag((counts[:, None] * g).sum(0)) + nhh) @ Q.T
        _C = Q @ hs
        _R = 0.5 * (e_hh + e_hh.T) / n_classes
        F = linalg.solve(0.5 * (_A + _A.T), _C).T
        Sigma = sigma_obs - F @ _C / n_total
        F = F @ linalg.cholesky(_R)          # scipy's UPPER factor, as speechbrain's minimum-divergence step
    return F, Sigma


def _labels(labels, n):
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"labels: expected {n} class labels, got shape {lab.shape}")
    classes, inv = np.unique(lab, return_inverse=True)      # sorted unique names: speechbrain's sum_stat_per_model order
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable").astype(np.int32)
    start = np.zeros(classes.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(inv, minlength=classes.shape[0]), out=start[1:])
    return classes, order, start


class PldaStats:
    """The N-scale pass of PLDA training, run once on a HIP device: `mean` [D], `sigma_obs` [D, D] (biased centred
    covariance, exactly symmetric), `counts` [C] (scaled class sizes), `classes` (sorted label names) on the host, the scaled
    centred class sums on the device.  `fit(rank_f, nb_iter)` runs the EM from them; fits of several ranks share the pass."""

    def __init__(self, x, labels, scaling_factor=1.0, device="cuda:0"):
        self.device = require_device(device, "PLDA training")
        t = dev_f64(x, self.device, keep_f32=True)
        if t.dim() != 2:
            raise ValueError(f"PldaStats: expected [N, D] x-vectors, got shape {tuple(t.shape)}")
        n, dim = int(t.shape[0]), int(t.shape[1])
        self.classes, order, start = _labels(labels, n)
        C = int(self.classes.shape[0])
        self.n, self.dim, self.n_classes = n, dim, C
        self.scaling_factor = float(scaling_factor)
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        mean = torch.empty(dim, **f64)
        counts = torch.empty(C, **f64)
        self._cls = torch.empty((C, dim), **f64)
        self._cls_t = torch.empty((dim, C), **f64)
        sigma = torch.empty((dim, dim), **f64)
        order_d = torch.from_numpy(order).to(dev)
        ws = byte_workspace(_hip.lib.xvec_plda_stats_workspace_bytes(n, dim, C), dev)
        xd = _hip.PLDA_X_F32 if t.dtype == torch.float32 else _hip.PLDA_X_F64
        with torch.cuda.device(dev):
            _check(_hip.lib.xvec_plda_stats(t.data_ptr(), xd, n, dim, order_d.data_ptr(), i64_ptr(start), C, self.scaling_factor,
                                            mean.data_ptr(), counts.data_ptr(), self._cls.data_ptr(), self._cls_t.data_ptr(),
                                            sigma.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
        self._counts = counts
        self._em_ws = None
        self.mean = mean.cpu().numpy()
        self.sigma_obs = sigma.cpu().numpy()
        self.counts = counts.cpu().numpy()
        self.last_fit_timing = None

    def class_sums(self) -> np.ndarray:
        """[C, D] scaled centred class sums (scaling * sum of the class's rows - counts * mean), numpy float64."""
        return self._cls.cpu().numpy()

    def products(self, pq, lam):
        """(H'H, H' diag(n) H, H' S~) on the device for one EM iteration (see host_em)."""
        dev, R = self.device, int(np.asarray(lam).shape[0])
        pq_t = dev_f64(np.asarray(pq).T, dev)
        lam_d = dev_f64(lam, dev)
        out = torch.empty((R, 2 * R + self.dim), dtype=torch.float64, device=dev)
        self._em_ws = byte_workspace(_hip.lib.xvec_plda_em_workspace_bytes(self.n_classes, R), dev, self._em_ws)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            _check(_hip.lib.xvec_plda_em_products(pq_t.data_ptr(), self._cls.data_ptr(), self._cls_t.data_ptr(),
                                                  self._counts.data_ptr(), lam_d.data_ptr(), self.n_classes, self.dim, R,
                                                  out.data_ptr(), self._em_ws.data_ptr(), self._em_ws.numel(), _stream(dev)))
            t1.record(s)
        o = out.cpu().numpy()
        self._device_ms += t0.elapsed_time(t1)
        return o[:, :R], o[:, R:2 * R], o[:, 2 * R:]

    def fit(self, rank_f, nb_iter=10):
        """(mean, F, Sigma), numpy float64: speechbrain's PLDA EM (default path) on these statistics."""
        if not 1 <= int(rank_f) <= self.dim:
            raise ValueError(f"rank_f = {rank_f} must lie in [1, dim = {self.dim}]")
        self._device_ms = 0.0
        w0 = time.perf_counter()
        F, Sigma = host_em(self.sigma_obs, self.counts, int(rank_f), int(nb_iter), self.products)
        wall = time.perf_counter() - w0
        self.last_fit_timing = {"wall_s": wall, "device_s": self._device_ms / 1e3, "host_s": wall - self._device_ms / 1e3}
        return self.mean.copy(), F, Sigma


class StatObject:
    """The fields of speechbrain's StatObject_SB that the reference builds and reads (plda_classifier.py:7-79):
    `modelset` (class name per row), `segset` (row ids), `stat0` [N, 1] (ones), `stat1` [N, D]."""

    def __init__(self, modelset, segset, stat1, stat0=None, start=None, stop=None):
        self.modelset = np.asarray(modelset, dtype=object)
        self.segset = np.asarray(segset, dtype=object)
        self.stat1 = stat1
        n = len(self.modelset)
        self.stat0 = np.ones((n, 1)) if stat0 is None else np.asarray(stat0)
        self.start = np.array([None] * n) if start is None else start
        self.stop = np.array([None] * n) if stop is None else stop

    # speechbrain's StatObject_SB conditioning methods.  Each runs on the device (include/xvec_lda.h, xvector_amd.lda) and,
    # where speechbrain changes stat1 in place, stores a numpy float64 result.

    def _stats(self, device):
        return PldaStats(self.stat1, self.modelset, device=device)

    def _transform(self, mean, w, normalize, device):
        from .lda import embed_transform
        self.stat1 = embed_transform(self.stat1, mean, w, normalize, device=device).cpu().numpy()

    def get_mean_stat1(self, device="cuda:0"):
        """[D] mean of stat1."""
        return self._stats(device).mean

    def get_total_covariance_stat1(self, device="cuda:0"):
        """[D, D] biased centred covariance of stat1."""
        return self._stats(device).sigma_obs

    def center_stat1(self, mu, device="cuda:0"):
        self._transform(mu, None, False, device)

    def rotate_stat1(self, R, device="cuda:0"):
        self._transform(None, R, False, device)

    def norm_stat1(self, device="cuda:0"):
        """Every row divided by max(its 2-norm, 1e-8)."""
        self._transform(None, None, True, device)

    def whiten_stat1(self, mu, sigma, device="cuda:0"):
        """Centre by mu and rotate by V diag(1 / sqrt(lam)) of a 2-D sigma (eigenvalues descending), or scale by
        1 / sqrt(sigma) for a 1-D (diagonal) sigma."""
        from .lda import whitening_matrix
        self._transform(mu, whitening_matrix(sigma), False, device)

    def get_lda_matrix_stat1(self, rank, device="cuda:0"):
        """[D, rank] LDA matrix of stat1 with modelset as the classes (lda.LdaStats.matrix)."""
        from .lda import LdaStats
        return LdaStats(self.stat1, self.modelset, device=device).matrix(rank)


def get_train_x_vec(train_xv, train_label, x_id_train):
    """plda_classifier.get_train_x_vec: modelset 'id<label>', segset the x-vector ids."""
    n = train_xv.shape[0]
    return StatObject(modelset=["id" + str(train_label[i]) for i in range(n)],
                      segset=[str(x_id_train[i]) for i in range(n)], stat1=train_xv)


def get_x_vec_stat(xv, id):
    """plda_classifier.get_x_vec_stat: every x-vector its own model (modelset == segset == the ids)."""
    sets = [str(id[i]) for i in range(xv.shape[0])]
    return StatObject(modelset=sets, segset=sets, stat1=xv)


class PLDA:
    """speechbrain.processing.PLDA_LDA.PLDA's surface as the reference uses it: `plda(stat)` trains `mean`, `F`, `Sigma`
    (numpy float64, what PldaScorer and scoring.plda_scores take); picklable."""

    def __init__(self, mean=None, F=None, Sigma=None, rank_f=150, nb_iter=10, scaling_factor=1.0, device="cuda:0"):
        self.mean = mean
        self.F = F
        self.Sigma = Sigma
        self.rank_f = rank_f
        self.nb_iter = nb_iter
        self.scaling_factor = scaling_factor
        self.device = str(device)

    def plda(self, stat_server=None, output_file_name=None, whiten=False, w_stat_server=None):
        if whiten or w_stat_server is not None:
            raise NotImplementedError("whiten=True / w_stat_server are not on the reference's path")
        stats = PldaStats(stat_server.stat1, stat_server.modelset, scaling_factor=self.scaling_factor, device=self.device)
        self.mean, self.F, self.Sigma = stats.fit(self.rank_f, self.nb_iter)
        if output_file_name is not None:
            save_plda(self, output_file_name)


def setup_plda(mean=None, F=None, Sigma=None, rank_f=150, nb_iter=10, scaling_factor=1, device="cuda:0"):
    """plda_classifier.setup_plda"""
    return PLDA(mean=mean, F=F, Sigma=Sigma, rank_f=rank_f, nb_iter=nb_iter, scaling_factor=scaling_factor, device=device)


def train_plda(plda, xvectors_stat):
    """plda_classifier.train_plda"""
    plda.plda(xvectors_stat)
    return plda


def lda(x_vec_stat, reduced_dim=2, device="cuda:0"):
    """plda_classifier.lda (xvector_amd.lda.lda)"""
    from .lda import lda as _lda
    return _lda(x_vec_stat, reduced_dim=reduced_dim, device=device)


def save_plda(plda, file_name):
    with open(file_name, "wb") as f:
        pickle.dump(plda, f)


def load_plda(file_name):
    with open(file_name, "rb") as f:
        return pickle.load(f)
