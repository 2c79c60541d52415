"""Speaker diarization on the GPU: who spoke when in recordings without enrolled speakers (include/xvec_diar.h).

The reference has no diarization; this is the x-vector recipe's step behind the scorer (Kaldi's callhome recipe): every
recording's window-by-window scores are clustered by agglomerative hierarchical clustering with average linkage, up to a score
threshold or down to a given number of speakers.  The kernels are checked against tests/diar_ref.py, a numpy restatement that
tests/test_diarize.py holds against scipy.cluster.hierarchy.linkage.  The score matrix stays where the scorer left it.

    S = scorer.score(window_xvecs)                          # [N, N] float64 on the device, every recording a diagonal block
    cl = cluster(S, rec_start, threshold=0.0)               # Clustering: .labels [N] int32, .n_clusters [n_rec] int32 (device)
    cl = cluster(S, rec_start, n_speakers=2)                # ... or down to a number of speakers (a sequence: per recording)

    d = Diarizer(model, scorer, transform, win=150, hop=75, threshold=0.0)
    res = d.diarize(x, lengths)                             # Diarization: .windows, .labels, .n_clusters, .turns (host)
    write_rttm(res.turns, names, "out.rttm")
    d = Diarizer(model, scorer, transform, frontend=vad.VadCmvn(), max_gap=10)      # the recipe's front end: sliding CMVN, and
                                                                                    # windows inside the runs of speech only
    d = Diarizer(model, scorer, transform, threshold=0.0, resegment=vbx.Vbx(vbx.VbxModel.from_plda(plda), n_speakers=10))
                                                                                    # VBx behind the clustering (vbx.py)

Largest score first, equal scores by the lowest pair of cluster indices, NaN never; clusters are numbered in the order of
their first window.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import hip as _hip
from ._device import (byte_workspace, checker, dev_f64, i64_ptr, rec_start as _dev_rec_start, require_device, score_matrix,
                      stream as _stream)

__all__ = ["cluster", "Clustering", "turns", "write_rttm", "Diarizer", "Diarization", "MAX_SEGMENTS", "THREADS_SMALL",
           "THREADS_LARGE", "RESCAN_WIDTH"]

# include/xvec_diar.h: the most segments of a recording, the threads of a small and of a large recording's block, the cells a
# wave reads at a time when it rescans a row
MAX_SEGMENTS, THREADS_SMALL, THREADS_LARGE, RESCAN_WIDTH = 2048, 64, 256, 64

_check = checker(_hip.lib.xvec_diar_last_error)
_I32P = _hip.C.POINTER(_hip.C.c_int32)


class Clustering(NamedTuple):
    labels: torch.Tensor                        # [N] int32: the cluster of every segment, 0 .. n_clusters[r] - 1 per recording
    n_clusters: torch.Tensor                    # [n_rec] int32
    merges: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]      # (i, j, score) [N]: the header's merge slots


def _matrix(scores, what) -> torch.Tensor:
    return score_matrix(scores, what, "[N, N]", square=True)


def _rec_start(rec_start, n, what) -> np.ndarray:
    return _dev_rec_start(rec_start, n, what, "rows of the score matrix", "segment")


def cluster(S, rec_start, threshold=None, n_speakers=None, max_speakers=None, return_merges=False, workspace=None) -> Clustering:
    """Average-linkage clustering of the diagonal blocks of the device score matrix S [N, N] (float64, unit column stride;
    only the cells above the diagonal inside a block are read), recording r being rows rec_start[r] .. rec_start[r + 1] - 1
    (host integers).  Merging stops at `threshold` (the best pair scores below it), never before `max_speakers` clusters or
    fewer are left; with `n_speakers` (an integer, or one per recording; 0 = by threshold) exactly when that many are left.
    At least one of `threshold` / `n_speakers` must be given."""
    s = _matrix(S, "cluster")
    n = int(s.shape[0])
    rs = _rec_start(rec_start, n, "cluster")
    n_rec = rs.shape[0] - 1
    if threshold is None and n_speakers is None:
        raise ValueError("cluster: give a threshold, n_speakers, or both")
    want = None
    if n_speakers is not None:
        want = np.ascontiguousarray(np.broadcast_to(np.asarray(n_speakers, dtype=np.int32), (n_rec,)))
        if (want < 0).any() or (threshold is None and (want < 1).any()):
            raise ValueError("cluster: n_speakers must be positive (0 = by threshold, where a threshold is given)")
    thr = float("inf") if threshold is None else float(threshold)
    if thr != thr:
        raise ValueError("cluster: the threshold is NaN")
    max_clusters = 0 if max_speakers is None else int(max_speakers)
    if max_clusters < 0:
        raise ValueError(f"cluster: max_speakers = {max_speakers} must not be negative")
    dev = s.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n_rec, dtype=torch.int32, device=dev)
    merges = None
    if return_merges:
        merges = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.float64, device=dev))
    rs_p = i64_ptr(rs)
    ws = byte_workspace(int(_hip.lib.xvec_ahc_workspace_bytes(rs_p, n_rec)), dev, workspace)
    with torch.cuda.device(dev):
        _check(_hip.lib.xvec_ahc_cluster(s.data_ptr(), s.stride(0), rs_p, n_rec, thr, max_clusters,
                                         None if want is None else want.ctypes.data_as(_I32P), labels.data_ptr(),
                                         counts.data_ptr(), *([None] * 3 if merges is None else [m.data_ptr() for m in merges]),
                                         ws.data_ptr(), ws.numel(), _stream(dev)))
    return Clustering(labels, counts, merges)


def turns(windows, labels) -> np.ndarray:
    """int64 [m, 4] rows (utt, start_frame, end_frame, speaker) of `windows` [n, 3] (utt, start, len) as extract_windows
    returns them -- grouped by recording, ascending in start -- and one label per window.  Two consecutive windows of a
    recording that overlap split the overlap at (start_b + start_a + len_a) // 2; without overlap each keeps its own span and
    the gap belongs to nobody.  Consecutive spans that touch and carry one label merge.  Host only."""
    w = np.asarray(windows.cpu().numpy() if isinstance(windows, torch.Tensor) else windows, dtype=np.int64).reshape(-1, 3)
    lab = np.asarray(labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels, dtype=np.int64).reshape(-1)
    if lab.shape[0] != w.shape[0]:
        raise ValueError(f"turns: {w.shape[0]} windows but {lab.shape[0]} labels")
    same = w[1:, 0] == w[:-1, 0]
    if (w[1:, 0] < w[:-1, 0]).any() or (same & (w[1:, 1] < w[:-1, 1])).any():
        raise ValueError("turns: the windows must be grouped by recording and ascending in start")
    start, end = w[:, 1].copy(), w[:, 1] + w[:, 2]
    for a in np.flatnonzero(same & (w[1:, 1] < end[:-1])):                 # window a overlaps its successor
        start[a + 1] = end[a] = (w[a + 1, 1] + w[a, 1] + w[a, 2]) // 2
    out = []
    for a in range(w.shape[0]):
        if end[a] <= start[a]:
            continue
        if out and out[-1][0] == w[a, 0] and out[-1][2] == start[a] and out[-1][3] == lab[a]:
            out[-1][2] = int(end[a])
        else:
            out.append([int(w[a, 0]), int(start[a]), int(end[a]), int(lab[a])])
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def write_rttm(turns, names, file, frame_shift=0.01) -> None:
    """One line `SPEAKER <name> 1 <onset> <dur> <NA> <NA> spk<k> <NA> <NA>` per turn, onset and duration in seconds with three
    decimals; names[utt] is the recording's name, `file` a path or an open text file."""
    lines = [f"SPEAKER {names[int(u)]} 1 {a * frame_shift:.3f} {(b - a) * frame_shift:.3f} <NA> <NA> spk{int(k)} <NA> <NA>\n"
             for u, a, b, k in np.asarray(turns, dtype=np.int64).reshape(-1, 4)]
    if hasattr(file, "write"):
        file.writelines(lines)
    else:
        with open(file, "w") as f:
            f.writelines(lines)


class Diarization(NamedTuple):
    windows: np.ndarray          # [n, 3] int32 (utt, start, len): the windows, as extract_windows returns them
    labels: np.ndarray           # [n] int32: the speaker of every window, numbered per recording in order of appearance
    n_clusters: np.ndarray       # [recordings with a window] int32
    turns: np.ndarray            # [m, 4] int64 (utt, start_frame, end_frame, speaker)


class Diarizer:
    """extract_windows -> transform -> score -> cluster on one HIP device.  `model`: an XVectorModel on the device; `scorer`:
    a `PldaScorer` or the string "cosine"; `transform`: an optional `EmbeddingTransform`; `win` / `hop` / `min_tail`: the
    sliding windows in frames (the recipe's 1.5 s every 0.75 s); `frontend`: an optional `vad.VadCmvn` -- the recordings are
    then normalised and windowed inside their runs of speech only (`max_gap`: the silence in frames a run bridges), as the
    recipe does, and the turns stay in the recordings' own frames.  Recordings are grouped into calls whose windows total at most
    `max_score_rows`: one call scores all its windows against each other (the scorer has no launch for the diagonal blocks
    alone), so the bound caps the cells computed between different recordings.  `resegment`: an optional `vbx.Vbx` -- the
    windows of each call then go through its model's projection and VBx, initialised from the clustering's labels (the
    clustering is capped at its n_speakers clusters through max_speakers), and the VBx labels replace the clustering's."""

    def __init__(self, model, scorer, transform=None, win=150, hop=75, threshold=None, max_speakers=None, min_tail=None,
                 max_score_rows=8192, device="cuda:0", frontend=None, max_gap=0, resegment=None):
        self.device = require_device(device, "diarization")
        if isinstance(scorer, str):
            if scorer != "cosine":
                raise ValueError(f"Diarizer: unknown scorer {scorer!r} (a PldaScorer or 'cosine')")
        elif not hasattr(scorer, "score"):
            raise TypeError("Diarizer: scorer must be a PldaScorer or the string 'cosine'")
        elif torch.device(scorer.device) != self.device:
            raise ValueError(f"Diarizer: the scorer lives on {scorer.device}, not on {self.device}")
        if int(max_score_rows) < 1:
            raise ValueError(f"Diarizer: max_score_rows = {max_score_rows} must be positive")
        self.model, self.scorer, self.transform = model, scorer, transform
        self.win, self.hop, self.min_tail = int(win), int(hop), min_tail
        self.threshold, self.max_speakers, self.max_score_rows = threshold, max_speakers, int(max_score_rows)
        if frontend is not None and not callable(getattr(frontend, "with_select", None)):
            raise TypeError("Diarizer: frontend must be a vad.VadCmvn")
        if int(max_gap) < 0:
            raise ValueError(f"Diarizer: max_gap = {max_gap} must not be negative")
        self.frontend, self.max_gap = frontend, int(max_gap)
        if resegment is not None:
            if not hasattr(resegment, "model") or not hasattr(resegment.model, "project"):
                raise TypeError("Diarizer: resegment must be a vbx.Vbx")
            cap = int(resegment.n_speakers)
            self.max_speakers = cap if self.max_speakers is None else min(int(self.max_speakers), cap)
        self.resegment = resegment
        self._ws = self._vbx_ws = None

    def _scores(self, v) -> torch.Tensor:
        if self.scorer == "cosine":
            from .scoring import cosine_scores
            return cosine_scores(v, device=self.device)
        return self.scorer.score(v)

    def _speech_windows(self, x, lengths):
        """extract_windows behind the front end: the recordings normalised where they lie (nothing selected, so a frame keeps
        its index), the windows inside the runs of speech -- gaps of at most max_gap frames closed, runs too short for a
        window dropped.  Without a VAD in the front end the windows cover the recordings."""
        from .vad import run_windows, speech_runs
        p = self.frontend.with_select(False)(x, lengths)
        if isinstance(p, torch.Tensor):
            return self.model.extract_windows(p, self.win, self.hop, lengths=lengths, min_tail=self.min_tail)
        shortest = self.win if self.min_tail is None else min(self.win, int(self.min_tail))
        windows = run_windows(speech_runs(p.mask, p.lengths, self.max_gap, shortest), self.win, self.hop, self.min_tail)
        if not len(windows):
            raise ValueError(f"Diarizer: no run of speech holds a window of {self.win} frames (min_tail={self.min_tail})")
        return self.model.extract_segments(p.feats, windows, lengths=p.lengths), windows

    def calls(self, rec_start):
        """[(first recording, one past the last)] of the scoring calls: consecutive recordings while their windows total at
        most max_score_rows (a recording with more windows than that is a call of its own).  Host arithmetic."""
        out, first = [], 0
        for r in range(1, len(rec_start)):
            if r > first + 1 and rec_start[r] - rec_start[first] > self.max_score_rows:
                out.append((first, r - 1))
                first = r - 1
        out.append((first, len(rec_start) - 1))
        return out

    def diarize(self, x, lengths=None, n_speakers=None) -> Diarization:
        """Diarize the recordings of x [B, T, C] (`lengths`: valid frames of each).  `n_speakers`: the number of speakers, one
        for all or one per recording of the batch (0 = by threshold); without it the Diarizer's threshold decides."""
        if self.threshold is None and n_speakers is None:
            raise ValueError("Diarizer: give a threshold at construction or n_speakers here")
        if self.frontend is None:
            vecs, windows = self.model.extract_windows(x, self.win, self.hop, lengths=lengths, min_tail=self.min_tail)
        else:
            vecs, windows = self._speech_windows(x, lengths)
        if self.transform is not None:
            vecs = self.transform.apply(vecs)
        vecs = dev_f64(vecs, self.device)
        utts, counts = np.unique(windows[:, 0], return_counts=True)           # (windows are ordered by recording)
        rec_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        want = None
        if n_speakers is not None:
            per_utt = np.broadcast_to(np.asarray(n_speakers, dtype=np.int32), (int(x.shape[0]),))
            want = per_utt[utts]
        labels = torch.empty(int(rec_start[-1]), dtype=torch.int32, device=self.device)
        n_clusters = torch.empty(len(utts), dtype=torch.int32, device=self.device)
        for a, b in self.calls(rec_start):
            lo, hi = int(rec_start[a]), int(rec_start[b])
            rs = rec_start[a:b + 1] - lo
            s = self._scores(vecs[lo:hi])
            self._ws = byte_workspace(int(_hip.lib.xvec_ahc_workspace_bytes(i64_ptr(rs), b - a)), self.device, self._ws)
            cl = cluster(s, rs, self.threshold, None if want is None else want[a:b], self.max_speakers, workspace=self._ws)
            if self.resegment is not None:
                from . import vbx as _vbx
                self._vbx_ws = byte_workspace(_vbx.workspace_bytes(rs, len(self.resegment.model.phi), self.resegment.n_speakers),
                                              self.device, self._vbx_ws)
                cl = _vbx.resegment(self.resegment, vecs[lo:hi], rs, cl.labels, self.device, workspace=self._vbx_ws)
                labels[lo:hi] = cl.labels
                n_clusters[a:b] = cl.n_speakers
                continue
            labels[lo:hi] = cl.labels
            n_clusters[a:b] = cl.n_clusters
        lab = labels.cpu().numpy()
        return Diarization(windows, lab, n_clusters.cpu().numpy(), turns(windows, lab))
