"""Trial-list evaluation on the GPU: the last stage of the reference's pipeline (main.py:312-336).

The reference picks the score of every line of `veri_test2.txt` out of the score matrix in a Python loop
(plda_score_stat.py:36-97) and hands the target and non-target scores to speechbrain's `EER` / `minDCF`, which walk every
candidate threshold over every trial.  Here the score matrix stays where `PldaScorer.score` / `cosine_scores` left it: the
trial scores are gathered, rounded to fp32 (the reference evaluates float32 tensors), sorted once by a radix sort written in
HIP, and both error rates of every threshold come off one prefix sum (include/xvec_eval.h).  A handful of numbers cross to
the host.

    trials = TrialList.from_file("veri_test2.txt", ids, ids)          # one dictionary per set, not a search per line
    res = evaluate_trials(scorer.score(x_vecs), trials, p_target=0.5) # TrialResult(eer, eer_th, far, frr, min_dcf, ...)
    res = evaluate_all_pairs(scorer.score(x_vecs), speaker_labels)    # every cell a trial, the diagonal skipped
    eer, th = EER(pos, neg); dcf, th = minDCF(pos, neg)               # drop-ins for speechbrain.utils.metric_stats
    st = plda_score_stat_object(x_vectors_test); st.test_plda(plda, path); st.calc_eer_mindcf()     # the reference's class

Parity with speechbrain itself is unpinned (not installed in the build image); tests/eer_ref.py restates its published
threshold walk and the kernels are checked against it.  One deviation: the error rates are exact here (integer counts,
fp64 quotients) where the package rounds them to fp32.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, dev_f64, require_device, score_matrix, sized_workspace, stream as _stream

__all__ = ["TrialList", "TrialResult", "evaluate_trials", "evaluate_all_pairs", "sorted_keys", "sorted_order", "EER", "minDCF",
           "plda_score_stat_object"]


class _Result(C.Structure):      # xvec_eval_result
    _fields_ = [("eer", C.c_double), ("eer_threshold", C.c_double), ("far", C.c_double), ("frr", C.c_double),
                ("min_dcf", C.c_double), ("min_dcf_threshold", C.c_double), ("n_target", C.c_int64),
                ("n_nontarget", C.c_int64), ("n_nan", C.c_int64), ("n_bad_index", C.c_int64)]


_check = checker(_hip.lib.xvec_eval_last_error)


@dataclass
class TrialResult:
    eer: float
    eer_th: float
    far: float
    frr: float
    min_dcf: float
    min_dcf_th: float
    n_target: int
    n_nontarget: int


def parse_trial_line(line: str):
    """(is_target, enrol id, test id) of one line of a VoxCeleb trial file, as plda_score_stat.py:65-67 reads it."""
    fields = line.split(" ")
    return bool(int(fields[0].rstrip().split(".")[0].strip())), fields[1].strip(), fields[2].strip()


def _first_positions(names) -> dict:
    pos = {}
    for i, n in enumerate(np.asarray(names).tolist()):
        pos.setdefault(n, i)           # an id that occurs twice resolves to its FIRST position, as np.where(...)[0][0]
    return pos


class TrialList:
    """Trials as positions in a score matrix: `row_idx` / `col_idx` (int32) and `is_target` (uint8), host arrays."""

    def __init__(self, row_idx, col_idx, is_target):
        self.row_idx = np.ascontiguousarray(np.asarray(row_idx), dtype=np.int32)
        self.col_idx = np.ascontiguousarray(np.asarray(col_idx), dtype=np.int32)
        self.is_target = np.ascontiguousarray(np.asarray(is_target).astype(bool), dtype=np.uint8)
        if not (self.row_idx.ndim == 1 and self.row_idx.shape == self.col_idx.shape == self.is_target.shape):
            raise ValueError("TrialList: row_idx, col_idx and is_target must be vectors of one length")
        self._dev = {}

    def __len__(self):
        return int(self.row_idx.shape[0])

    @classmethod
    def from_file(cls, path, modelset, segset):
        """The reference's trial file (`<label> <enrol id> <test id>` per line; the label `1`, `0` or spelt `1.0`) against the
        ids of the score matrix's rows (`modelset`) and columns (`segset`).  An id missing from its set raises KeyError."""
        rows_of, cols_of = _first_positions(modelset), _first_positions(segset)
        rows, cols, labels = [], [], []
        with open(path) as f:
            for line in f:
                if not line.strip():
                    continue
                match, enrol_id, test_id = parse_trial_line(line)
                if enrol_id not in rows_of:
                    raise KeyError(f"trial file {path}: enrolment id {enrol_id!r} is not in the model set")
                if test_id not in cols_of:
                    raise KeyError(f"trial file {path}: test id {test_id!r} is not in the segment set")
                rows.append(rows_of[enrol_id])
                cols.append(cols_of[test_id])
                labels.append(match)
        return cls(rows, cols, labels)

    def on(self, device):
        """(row_idx, col_idx, is_target) on `device`; copied once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.row_idx, self.col_idx, self.is_target))
        return self._dev[key]


def _matrix(scoremat) -> torch.Tensor:
    return score_matrix(scoremat, "trial evaluation")


def _workspace(n: int, device) -> torch.Tensor:
    refusal = lambda: ValueError(f"{n} trials: the count must lie in 1 .. 2^31 - 1")
    return sized_workspace(_hip.lib.xvec_eval_workspace_bytes(n), refusal, device)


def trial_args(s: torch.Tensor, trials, what: str):
    """(row, col, is_target, n) on the scores' device; `trials` a TrialList, or for a score VECTOR the target flags alone."""
    if isinstance(trials, TrialList):
        if len(trials) < 1:
            raise ValueError(f"{what}: no trials")
        row, col, tgt = trials.on(s.device)
        return row, col, tgt, len(trials)
    tgt = torch.as_tensor(trials).to(device=s.device).ne(0).to(torch.uint8).contiguous()
    if s.shape[0] != 1 or tgt.dim() != 1 or tgt.numel() != s.shape[1] or tgt.numel() < 1:
        raise ValueError(f"{what}: target flags alone go with a score vector of their length (a TrialList indexes a matrix)")
    return None, None, tgt, tgt.numel()


def score_vector_or_matrix(scores, what: str) -> torch.Tensor:
    """A device score matrix, or a device score vector as the [1, n] matrix the plain-vector form reads."""
    if isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() == 1 and scores.dtype == torch.float64:
        scores = scores.reshape(1, -1)
    return score_matrix(scores, what)


def _read_result(out: torch.Tensor, what: str) -> TrialResult:
    r = _Result.from_buffer_copy(out.cpu().numpy().tobytes())          # the one copy to the host: 80 bytes
    if r.n_bad_index:
        raise IndexError(f"{what}: {r.n_bad_index} trial(s) point outside the score matrix")
    if r.n_nan:
        raise ValueError(f"{what}: {r.n_nan} trial score(s) are NaN")
    if r.n_target == 0 or r.n_nontarget == 0:
        raise ValueError(f"{what}: {r.n_target} target and {r.n_nontarget} non-target trials; both kinds are needed")
    return TrialResult(r.eer, r.eer_threshold, r.far, r.frr, r.min_dcf, r.min_dcf_threshold, int(r.n_target),
                       int(r.n_nontarget))


def _eval(scores, ld, n_rows, n_cols, row, col, tgt, n, c_miss, c_fa, p_target, what, workspace=None) -> TrialResult:
    device = scores.device
    ws = _workspace(n, device) if workspace is None else workspace
    out = torch.empty(len(_Result._fields_), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_eval_trials(scores.data_ptr(), ld, n_rows, n_cols, None if row is None else row.data_ptr(),
                                         None if col is None else col.data_ptr(), tgt.data_ptr(), n, float(c_miss),
                                         float(c_fa), float(p_target), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream(device)))
    return _read_result(out, what)


def evaluate_trials(scoremat, trials: TrialList, c_miss=1.0, c_fa=1.0, p_target=0.5, workspace=None) -> TrialResult:
    """EER and minDCF of `trials` over the device score matrix (float64, as PldaScorer.score leaves it; it stays there)."""
    s = _matrix(scoremat)
    if len(trials) < 1:
        raise ValueError("evaluate_trials: no trials")
    row, col, tgt = trials.on(s.device)
    return _eval(s, s.stride(0), s.shape[0], s.shape[1], row, col, tgt, len(trials), c_miss, c_fa, p_target,
                 "evaluate_trials", workspace)


def _class_ids(labels, others=None):
    """int32 class ids of arbitrary labels (equal labels <-> equal ids), shared between rows and columns."""
    a = np.asarray(labels)
    if others is None:
        return np.unique(a, return_inverse=True)[1].astype(np.int32), None
    b = np.asarray(others)
    inv = np.unique(np.concatenate([a, b]), return_inverse=True)[1].astype(np.int32)
    return inv[: len(a)], inv[len(a):]


def evaluate_all_pairs(scoremat, row_labels, col_labels=None, skip_diagonal=True, c_miss=1.0, c_fa=1.0, p_target=0.5,
                       workspace=None) -> TrialResult:
    """Every cell of the score matrix as a trial: a target iff the row's and the column's label are equal.  `col_labels=None`
    takes the row labels (a set against itself); `skip_diagonal` leaves the cells i == j out."""
    s = _matrix(scoremat)
    n_rows, n_cols = s.shape
    rc, cc = _class_ids(row_labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != n_rows or len(cc) != n_cols:
        raise ValueError(f"evaluate_all_pairs: {len(rc)} row and {len(cc)} column labels for a {n_rows} x {n_cols} matrix")
    n = n_rows * n_cols
    ws = _workspace(n, s.device) if workspace is None else workspace
    rcd, ccd = torch.from_numpy(rc).to(s.device), torch.from_numpy(cc).to(s.device)
    out = torch.empty(len(_Result._fields_), dtype=torch.float64, device=s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_eval_all_pairs(s.data_ptr(), s.stride(0), n_rows, n_cols, rcd.data_ptr(), ccd.data_ptr(),
                                            int(bool(skip_diagonal)), float(c_miss), float(c_fa), float(p_target),
                                            out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(s.device)))
    return _read_result(out, "evaluate_all_pairs")


def sorted_keys(scores, is_target, workspace=None):
    """The sort alone, for inspection and tests: (keys uint32 as int64 tensor, bits uint8) of a device vector of float64 trial
    scores, sorted as the evaluation sorts them (include/xvec_eval.h, xvec_eval_sorted_keys)."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise RuntimeError("trial evaluation runs on a HIP device only (no CPU path)")
    s = scores.to(torch.float64).contiguous().reshape(-1)
    n = s.numel()
    tgt = torch.as_tensor(is_target).to(device=s.device, dtype=torch.uint8).contiguous()
    if tgt.numel() != n:
        raise ValueError("sorted_keys: one target flag per score")
    ws = _workspace(n, s.device) if workspace is None else workspace
    keys = torch.empty(n, dtype=torch.int32, device=s.device)
    bits = torch.empty(n, dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_eval_sorted_keys(s.data_ptr(), n, 1, n, None, None, tgt.data_ptr(), n, keys.data_ptr(),
                                              bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream(s.device)))
    return keys.to(torch.int64) & 0xFFFFFFFF, bits


def sorted_order(scores, is_target, workspace=None):
    """The sort with the trial's place as its payload (include/xvec_eval.h, xvec_eval_sorted_order): (keys uint32 as int64
    tensor, order as int64 tensor) of a device vector of float64 trial scores.  order[k] is the index of the trial at sorted
    position k; the sort is stable, so trials of equal key keep the order of their indices."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise RuntimeError("trial evaluation runs on a HIP device only (no CPU path)")
    s = scores.to(torch.float64).contiguous().reshape(-1)
    n = s.numel()
    tgt = torch.as_tensor(is_target).to(device=s.device, dtype=torch.uint8).contiguous()
    if tgt.numel() != n:
        raise ValueError("sorted_order: one target flag per score")
    refusal = lambda: ValueError(f"{n} trials: the count must lie in 1 .. 2^31 - 1")
    ws = sized_workspace(_hip.lib.xvec_eval_sorted_order_workspace_bytes(n), refusal, s.device, workspace)
    keys = torch.empty(n, dtype=torch.int32, device=s.device)
    order = torch.empty(n, dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_eval_sorted_order(s.data_ptr(), n, 1, n, None, None, tgt.data_ptr(), n, keys.data_ptr(),
                                               order.data_ptr(), ws.data_ptr(), ws.numel(), _stream(s.device)))
    return keys.to(torch.int64) & 0xFFFFFFFF, order.to(torch.int64) & 0xFFFFFFFF


def _score_vector(scores, device):
    """Scores as the reference feeds them to the package: float32 values (round to nearest even), here held as float64."""
    if isinstance(scores, torch.Tensor) and scores.is_cuda:
        device = scores.device
    return dev_f64(scores, device).reshape(-1).to(torch.float32).to(torch.float64), device


def _pos_neg(positive_scores, negative_scores, c_miss, c_fa, p_target, device, what) -> TrialResult:
    device = require_device(device, "trial evaluation")
    pos, device = _score_vector(positive_scores, device)
    neg, device = _score_vector(negative_scores, device)
    device = require_device(device, "trial evaluation")
    if pos.numel() == 0 or neg.numel() == 0:
        raise ValueError(f"{what}: {pos.numel()} positive and {neg.numel()} negative scores; both kinds are needed")
    s = torch.cat([pos, neg.to(device)])
    tgt = torch.zeros(s.numel(), dtype=torch.uint8, device=device)
    tgt[: pos.numel()] = 1
    return _eval(s, s.numel(), 1, s.numel(), None, None, tgt, s.numel(), c_miss, c_fa, p_target, what)


def EER(positive_scores, negative_scores, device="cuda:0"):
    """speechbrain.utils.metric_stats.EER: (equal error rate, its threshold).  Tensors, arrays or lists; the scores are moved
    to the device and rounded to float32, which is what the reference passes (plda_score_stat.py:96)."""
    r = _pos_neg(positive_scores, negative_scores, 1.0, 1.0, 0.5, device, "EER")
    return r.eer, r.eer_th


def minDCF(positive_scores, negative_scores, c_miss=1.0, c_fa=1.0, p_target=0.01, device="cuda:0"):
    """speechbrain.utils.metric_stats.minDCF with its defaults: (minimum detection cost, its threshold)."""
    r = _pos_neg(positive_scores, negative_scores, c_miss, c_fa, p_target, device, "minDCF")
    return r.min_dcf, r.min_dcf_th


class plda_score_stat_object:
    """The reference's class (plda_score_stat.py:13-97) with the same attributes after the same calls.  `x_vectors_test` is
    the DataFrame the reference reads from x_vector_test.csv (column 1 the ids, column 3 the vectors in numpy's print form).
    Scoring, the gather of the trial scores and the evaluation run on `device`; the trial scores come back to the host (the
    matrix does not, unless `plda_scores` is read)."""

    def __init__(self, x_vectors_test, device="cuda:0"):
        from . import plda as _plda
        self.device = require_device(device, "trial evaluation")
        self.x_vectors_test = x_vectors_test
        self.x_id_test = np.array(self.x_vectors_test.iloc[:, 1])
        self.x_vec_test = np.array([np.array(x_vec[1:-1].split(), dtype=np.float64)
                                    for x_vec in self.x_vectors_test.iloc[:, 3]])
        self.en_stat = _plda.get_x_vec_stat(self.x_vec_test, self.x_id_test)
        self.te_stat = _plda.get_x_vec_stat(self.x_vec_test, self.x_id_test)

        self._plda_scores = 0
        self._scoremat = None
        self._trials = None
        self.positive_scores = []
        self.negative_scores = []
        self.positive_scores_mask = []
        self.negative_scores_mask = []

        self._evaluated = False
        self.eer = 0
        self.eer_th = 0
        self.min_dcf = 0
        self.min_dcf_th = 0

        self.checked_xvec = []
        self.checked_label = []

    @property
    def plda_scores(self):
        """The host `Scores` object the reference keeps (modelset, segset, scoremat): built on first access."""
        if self._plda_scores == 0 and self._scoremat is not None:
            from .scoring import Scores
            self._plda_scores = Scores(self.en_stat.modelset, self.te_stat.modelset, self._scoremat.cpu().numpy())
        return self._plda_scores

    def test_plda(self, plda, veri_test_file_path, cohort=None, top_k=0):
        """Scores every test x-vector against every other one with `plda` (.mean, .F, .Sigma) and collects the trials of the
        VoxCeleb trial file.  With `cohort` ([C, D] x-vectors; not in the reference) the score matrix is S-normalised on the
        device against it before the trials are gathered (adaptive S-norm over the `top_k` largest cohort scores of every
        vector when top_k > 0: snorm.ScoreNormalizer); the default leaves every attribute as the reference computes it."""
        from .scoring import PldaScorer
        scorer = PldaScorer(plda.mean, plda.F, plda.Sigma, device=self.device)
        self._scoremat = scorer.score(self.x_vec_test)       # en_stat and te_stat hold the same vectors: the self path
        if cohort is not None:
            from .snorm import ScoreNormalizer
            norm = ScoreNormalizer(scorer, cohort, top_k=top_k, device=self.device)
            norm.normalize(self._scoremat, self.x_vec_test, mode="s", out=self._scoremat)
        self._plda_scores = 0
        modelset, segset = self.en_stat.modelset, self.te_stat.modelset
        self._trials = trials = TrialList.from_file(veri_test_file_path, modelset, segset)
        row, col, _ = trials.on(self.device)
        picked = self._scoremat[row.long(), col.long()].cpu().numpy()
        match = trials.is_target.astype(bool)
        self.positive_scores.extend(picked[match].tolist())
        self.negative_scores.extend(picked[~match].tolist())
        n = (len(modelset), len(segset))
        self.positive_scores_mask = np.zeros(n, dtype=np.float64)
        self.negative_scores_mask = np.zeros(n, dtype=np.float64)
        self.positive_scores_mask[trials.row_idx[match], trials.col_idx[match]] = 1
        self.negative_scores_mask[trials.row_idx[~match], trials.col_idx[~match]] = 1
        # the x-vectors and speaker numbers of the ids the file names, in order of first appearance (enrol id, then test id)
        seen = {}
        for r, c in zip(trials.row_idx.tolist(), trials.col_idx.tolist()):
            seen.setdefault(modelset[r], r)
            seen.setdefault(segset[c], c)
        xvec = list(self.checked_xvec) + [self.x_vec_test[i] for i in seen.values()]
        label = list(self.checked_label) + [int(name.split(".")[0].split("/")[0][2:]) for name in seen]
        self.checked_xvec = np.array(xvec)
        self.checked_label = np.array(label)

    def calc_eer_mindcf(self):
        """EER and minDCF (p_target = 0.5, as the reference calls it) of the collected trials."""
        if self._trials is None:
            raise RuntimeError("calc_eer_mindcf: call test_plda first")
        res = evaluate_trials(self._scoremat, self._trials, p_target=0.5)
        self.eer, self.eer_th = res.eer, res.eer_th
        self.min_dcf, self.min_dcf_th = res.min_dcf, res.min_dcf_th
        self._evaluated = True

    def confidence(self, n_boot=1000, seed=0, level=0.95):
        """Bootstrap confidence intervals of the collected trials' EER and minDCF over the SPEAKERS of the two trial sides
        (bootstrap.bootstrap_trials, joint: enrolment and test ids are one set, so one resample of its speakers weighs both
        sides).  The speaker of an id is the directory it starts with, as `checked_label` reads it.  Returns the
        BootstrapResult; `eer_ci` and `min_dcf_ci` hold the (lo, hi) intervals at `level`.  Call test_plda first."""
        from . import bootstrap
        s, trials = self._scored("confidence")
        speaker = lambda names: [name.split(".")[0].split("/")[0] for name in np.asarray(names).tolist()]
        boot = bootstrap.bootstrap_trials(s, trials, row_groups=speaker(self.en_stat.modelset),
                                          col_groups=speaker(self.te_stat.modelset), joint=True, n_boot=n_boot, seed=seed,
                                          p_target=0.5)
        self.eer_ci = boot.interval("eer", level)
        self.min_dcf_ci = boot.interval("min_dcf", level)
        return boot

    def analyze(self, k=200, bins=None):
        """What extra/compare_speaker_results.py looks at, for the collected trials, on the device (analyze.score_summary and
        analyze.hardest_trials): returns (ScoreSummary, HardestTrials) and keeps them as `score_summary` / `hardest`.  `bins`:
        an analyze.Bins for the histograms of the rounded scores, or None.  Call test_plda first."""
        from . import analyze as _analyze
        s, trials = self._scored("analyze")
        self.score_summary = _analyze.score_summary(s, trials, bins=bins)
        self.hardest = _analyze.hardest_trials(s, trials, k=k)
        return self.score_summary, self.hardest

    def _scored(self, what, thresholds=False):
        if self._trials is None:
            raise RuntimeError(f"{what}: call test_plda first")
        if thresholds and not self._evaluated:
            raise RuntimeError(f"{what}: call calc_eer_mindcf first")
        return self._scoremat, self._trials

    def score_images(self, dtype=torch.uint8):
        """The six images of the reference's plot_images (plda_score_stat.py:132-192) at the object's own thresholds, on the
        device, by the reference's names (report.score_images).  Call test_plda and calc_eer_mindcf first."""
        from . import report
        s, trials = self._scored("score_images", thresholds=True)
        return report.score_images(s, trials, self.eer_th, self.min_dcf_th, dtype=dtype)

    def det_curve(self, grid=0):
        """The error-rate curve of the collected trials (report.det_curve): every distinct score, or thinned to `grid`."""
        from . import report
        s, trials = self._scored("det_curve")
        return report.det_curve(s, trials, grid)

    def write_images(self, writer, step=0):
        """`writer.add_image(name, image, step)` for the six images in the reference's order: the image half of plot_images,
        for a TensorBoard SummaryWriter or any object with `add_image`.  The images cross to the host as uint8."""
        from . import report
        images = self.score_images()
        for name in report.IMAGE_NAMES:
            writer.add_image(name, images[name].cpu(), step)

    def plot_images(self, writer):
        raise NotImplementedError("plot_images (TensorBoard images, LDA / PCA / t-SNE scatter plots) is out of scope")
