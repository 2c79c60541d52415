"""Trial report on the GPU: the score-matrix images of the reference's plot_images and the DET curve (include/xvec_report.h).

The reference turns the score matrix, the trial masks and the two thresholds into six TensorBoard images in numpy
(plda_score_stat.py:132-192), each a [3, N, 2N + 5] float64 array, and gives two operating points and no curve.  Here the
matrix stays where `PldaScorer.score` left it: the trial list becomes a byte map of the matrix, one pass writes every image
as uint8 (what the TensorBoard writer makes of a float image) or float32, and the error rates of every distinct score come off
the sorted keys the evaluation already computes.

    m = trial_map(trials, S.shape, S.device)                         # uint8 [R, C]: bit 0 target, bit 1 non-target
    imgs = score_images(S, trials, res.eer_th, res.min_dcf_th)       # {name: uint8 tensor [3, R, C] or [3, R, 2C + 5]}
    det = det_curve(S, trials, grid=1000)                            # DetCurve: thresholds, tp, nn, far, frr, eer(), min_dcf()
    rep = trial_report(S, trials)                                    # TrialReport(result, det, images)
    st = plda_score_stat_object(...); ...; st.write_images(writer)   # the switch-over from plot_images

Deviations from the reference (include/xvec_report.h): the range of the score matrix leaves non-finite cells out; parity of the
uint8 rule with torch.utils.tensorboard is unpinned.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, ptr as _p, score_matrix, sized_workspace, stream as _stream
from .evaluate import TrialList, TrialResult, _class_ids, evaluate_trials, score_vector_or_matrix, trial_args

__all__ = ["DetCurve", "TrialReport", "trial_map", "score_range", "score_images", "det_curve", "det_curve_all_pairs",
           "trial_report", "IMAGE_NAMES", "SCORE_MATRIX", "GROUND_TRUTH", "GROUND_TRUTH_SCORES", "PREDICTION", "CORRECT", "FALSE",
           "ALL", "THREADS", "TILE", "RANGE_BLOCKS", "DET_ITEMS", "DET_TILE", "GAP"]

# include/xvec_report.h
THREADS, TILE, RANGE_BLOCKS, DET_ITEMS, DET_TILE, GAP = 256, 4096, 1024, 16, 4096, 5
U8, F32 = 0, 1
SCORE_MATRIX, GROUND_TRUTH, GROUND_TRUTH_SCORES, PREDICTION, CORRECT, FALSE, ALL = 1, 2, 4, 8, 16, 32, 63
# the reference's names, in the order it writes them (plda_score_stat.py:142-192); bit i of `which` selects IMAGE_NAMES[i]
IMAGE_NAMES = ("score_matrix", "ground_truth", "ground_truth_scores", "prediction_eer_min_dcf", "correct_prediction_eer_min_dcf",
               "false_prediction_eer_min_dcf")

_check = checker(_hip.lib.xvec_report_last_error)


class _Range(C.Structure):       # xvec_report_range_result
    _fields_ = [("min", C.c_double), ("max", C.c_double), ("n_nonfinite", C.c_int64)]


class _Header(C.Structure):      # xvec_report_det_header
    _fields_ = [("n_points", C.c_int64), ("n_target", C.c_int64), ("n_nontarget", C.c_int64), ("n_nan", C.c_int64),
                ("n_bad_index", C.c_int64)]


@dataclass
class DetCurve:
    """One point per distinct fp32 score, ascending (thinned when `grid` > 0): host arrays."""
    thresholds: np.ndarray       # float32 [n_points]
    tp: np.ndarray               # int64: targets at or below the threshold
    nn: np.ndarray               # int64: non-targets at or below it
    n_target: int
    n_nontarget: int
    n_nan: int
    n_bad_index: int
    grid: int = 0

    @property
    def frr(self) -> np.ndarray:
        """Targets rejected / targets: exact fp64 quotients (NaN without targets), as include/xvec_eval.h."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.tp.astype(np.float64) / np.float64(self.n_target)

    @property
    def far(self) -> np.ndarray:
        """Non-targets accepted / non-targets."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.n_nontarget - self.nn).astype(np.float64) / np.float64(self.n_nontarget)

    def _both_kinds(self, what):
        if self.n_target == 0 or self.n_nontarget == 0 or len(self.tp) == 0:
            raise ValueError(f"{what}: {self.n_target} target and {self.n_nontarget} non-target trials; both kinds are needed")

    def eer(self):
        """(EER, its threshold) recomputed from the points: arg-min of |(N - nn) P - tp N| in integers, the lowest threshold on
        ties -- `evaluate_trials`' values when the curve is not thinned."""
        self._both_kinds("DetCurve.eer")
        gap = np.abs((self.n_nontarget - self.nn) * self.n_target - self.tp * self.n_nontarget)
        k = int(np.argmin(gap))
        return float((self.far[k] + self.frr[k]) / 2.0), float(self.thresholds[k])

    def min_dcf(self, c_miss=1.0, c_fa=1.0, p_target=0.5):
        """(minimum detection cost, its threshold) recomputed from the points on the host, in the evaluation's order of
        operations.  `evaluate_trials`' value bit for bit where every product of the cost is exact (costs and a prior that are
        powers of two, as the reference's p_target = 0.5); elsewhere the device may fuse the sum that numpy rounds twice, and
        the two can differ in the last bit."""
        self._both_kinds("DetCurve.min_dcf")
        cost = c_miss * self.frr * p_target + c_fa * self.far * (1.0 - p_target)
        k = int(np.argmin(cost))
        return float(cost[k]), float(self.thresholds[k])


@dataclass
class TrialReport:
    result: TrialResult
    det: DetCurve
    images: dict


def _as_map(trials_or_map, s: torch.Tensor, what: str) -> torch.Tensor:
    if isinstance(trials_or_map, TrialList):
        return trial_map(trials_or_map, s.shape, s.device)
    m = trials_or_map
    if (not isinstance(m, torch.Tensor) or m.device != s.device or m.dtype != torch.uint8 or m.shape != s.shape or m.stride(1) != 1
            or m.stride(0) % 4 != 0 or m.data_ptr() % 4 != 0):
        raise ValueError(f"{what}: expected a TrialList or the uint8 map trial_map made for this matrix")
    return m


def trial_map(trials: TrialList, shape, device, return_bad=False):
    """The trial list as a uint8 [n_rows, n_cols] map on `device` (a view of a buffer whose rows are padded to whole 32-bit
    words): bit 0 of a cell is set if a target trial names it, bit 1 if a non-target trial does.  Trials that point outside
    the matrix touch no cell; `return_bad=True` returns (map, their count)."""
    n_rows, n_cols = (int(v) for v in shape)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the trial report runs on a HIP device only (no CPU path)")
    if n_rows < 1 or n_cols < 1:
        raise ValueError("trial_map: empty score matrix")
    ld = (n_cols + 3) // 4 * 4
    buf = torch.empty((n_rows, ld), dtype=torch.uint8, device=device)
    bad = torch.empty(1, dtype=torch.int64, device=device)
    row, col, tgt = trials.on(device) if len(trials) else (None, None, None)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_report_trial_map(_p(row), _p(col), _p(tgt), len(trials), n_rows, n_cols, buf.data_ptr(), ld,
                                              bad.data_ptr(), _stream(device)))
    m = buf[:, :n_cols]
    return (m, int(bad.item())) if return_bad else m


def _range_record(s: torch.Tensor) -> torch.Tensor:
    rec = torch.empty(C.sizeof(_Range) // 8, dtype=torch.float64, device=s.device)
    ws = torch.empty(int(_hip.lib.xvec_report_range_workspace_bytes()), dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_report_range(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], rec.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream(s.device)))
    return rec


def score_range(scoremat):
    """(minimum, maximum, count of non-finite cells) of the device score matrix; the range is that of the finite cells."""
    r = _Range.from_buffer_copy(_range_record(score_matrix(scoremat, "score_range")).cpu().numpy().tobytes())
    return r.min, r.max, int(r.n_nonfinite)


def _image_shape(i, n_rows, n_cols):
    return (n_rows, n_cols) if i == 0 else (3, n_rows, n_cols if i < 3 else 2 * n_cols + GAP)


def score_images(scoremat, trials_or_map, eer_th, min_dcf_th, dtype=torch.uint8, which=ALL, out=None) -> dict:
    """The reference's six images (those `which` selects) of the device score matrix, by name.  `score_matrix` is stored as one
    plane and returned as an expanded [3, R, C] view; the others are contiguous [3, R, C] and [3, R, 2C + 5] tensors.  `out`
    may hold tensors to write into, by name: contiguous, of `dtype`, of the stored shape ([R, C] for `score_matrix`)."""
    s = score_matrix(scoremat, "score_images")
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"score_images: dtype {dtype} is neither torch.uint8 nor torch.float32")
    which = int(which)
    if which <= 0 or which & ~ALL:
        raise ValueError(f"score_images: which = {which:#x} selects no image or an unknown one (bits {ALL:#x})")
    m = _as_map(trials_or_map, s, "score_images")
    n_rows, n_cols = s.shape
    rec = _range_record(s)
    stored = []
    for i, name in enumerate(IMAGE_NAMES):
        t = None
        if which >> i & 1:
            shape = _image_shape(i, n_rows, n_cols)
            t = (out or {}).get(name)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=s.device)
            elif (not isinstance(t, torch.Tensor) or t.device != s.device or t.dtype != dtype or tuple(t.shape) != shape
                  or not t.is_contiguous()):
                raise ValueError(f"score_images: out[{name!r}] must be a contiguous {dtype} device tensor of shape {shape}")
        stored.append(t)
    with torch.cuda.device(s.device):
        _check(_hip.lib.xvec_report_images(s.data_ptr(), s.stride(0), n_rows, n_cols, m.data_ptr(), m.stride(0), rec.data_ptr(),
                                           float(eer_th), float(min_dcf_th), which, U8 if dtype == torch.uint8 else F32,
                                           *[_p(t) for t in stored], _stream(s.device)))
    images = {name: t for name, t in zip(IMAGE_NAMES, stored) if t is not None}
    if "score_matrix" in images:
        images["score_matrix"] = images["score_matrix"].unsqueeze(0).expand(3, n_rows, n_cols)
    return images


def _curve(call, n, grid, device, workspace, *args) -> DetCurve:
    grid = int(grid)
    if not 0 <= grid <= 2 ** 31 - 1:
        raise ValueError(f"det_curve: grid = {grid} must lie in 0 .. 2^31 - 1")
    refusal = lambda: ValueError(f"{n} trials: the count must lie in 1 .. 2^31 - 1")
    ws = sized_workspace(_hip.lib.xvec_report_det_workspace_bytes(n), refusal, device, workspace)
    cap = n if grid == 0 else min(n, 2 * grid + 2)
    head = torch.empty(C.sizeof(_Header) // 8, dtype=torch.int64, device=device)
    thr = torch.empty(cap, dtype=torch.float32, device=device)
    tp = torch.empty(cap, dtype=torch.int64, device=device)
    nn = torch.empty(cap, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _check(call(*args, grid, head.data_ptr(), thr.data_ptr(), tp.data_ptr(), nn.data_ptr(), cap, ws.data_ptr(), ws.numel(),
                    _stream(device)))
    h = _Header.from_buffer_copy(head.cpu().numpy().tobytes())
    k = min(int(h.n_points), cap)
    return DetCurve(thr[:k].cpu().numpy(), tp[:k].cpu().numpy(), nn[:k].cpu().numpy(), int(h.n_target), int(h.n_nontarget),
                    int(h.n_nan), int(h.n_bad_index), grid)


def det_curve(scoremat, trials, grid=0, workspace=None) -> DetCurve:
    """The error-rate curve of `trials` (a TrialList over the device score matrix; or the target flags of a device score
    vector).  `grid` = G > 0 thins it to the points at which floor(G * FRR) or floor(G * FAR) steps (at most 2G + 2); 0 keeps
    every distinct score.  Trials with a NaN score or a bad index are counted in the curve and left out."""
    s = score_vector_or_matrix(scoremat, "det_curve")
    row, col, tgt, n = trial_args(s, trials, "det_curve")
    return _curve(_hip.lib.xvec_report_det, n, grid, s.device, workspace, s.data_ptr(), s.stride(0), s.shape[0], s.shape[1],
                  _p(row), _p(col), tgt.data_ptr(), n)


def det_curve_all_pairs(scoremat, row_labels, col_labels=None, skip_diagonal=True, grid=0, workspace=None) -> DetCurve:
    """det_curve over every cell of the matrix: a target iff the row's and the column's label are equal."""
    s = score_matrix(scoremat, "det_curve_all_pairs")
    rc, cc = _class_ids(row_labels, col_labels)
    if cc is None:
        cc = rc
    if len(rc) != s.shape[0] or len(cc) != s.shape[1]:
        raise ValueError(f"det_curve_all_pairs: {len(rc)} row and {len(cc)} column labels for a {s.shape[0]} x {s.shape[1]} matrix")
    rcd, ccd = torch.from_numpy(rc).to(s.device), torch.from_numpy(cc).to(s.device)
    return _curve(_hip.lib.xvec_report_det_all_pairs, s.shape[0] * s.shape[1], grid, s.device, workspace, s.data_ptr(),
                  s.stride(0), s.shape[0], s.shape[1], rcd.data_ptr(), ccd.data_ptr(), int(bool(skip_diagonal)))


def trial_report(scoremat, trials: TrialList, c_miss=1.0, c_fa=1.0, p_target=0.5, grid=0, dtype=torch.uint8,
                 which=ALL) -> TrialReport:
    """`evaluate_trials`, the DET curve and the images at the two thresholds it found, of one trial list over one device
    score matrix."""
    s = score_matrix(scoremat, "trial_report")
    res = evaluate_trials(s, trials, c_miss, c_fa, p_target)
    return TrialReport(res, det_curve(s, trials, grid), score_images(s, trials, res.eer_th, res.min_dcf_th, dtype, which))
