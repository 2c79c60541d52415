"""Voice activity detection and sliding-window CMVN on the GPU: the two steps between the MFCC front end and the extractor in
every Kaldi-style x-vector recipe (include/xvec_vad.h).

The reference has neither.  The energy VAD is Kaldi's compute-vad-decision, the normalisation its apply-cmvn-sliding, the
selection its select-voiced-frames -- all three RESTATED from memory: parity with Kaldi is UNPINNED (neither Kaldi nor a port
of it is installed where this was written).  The header is the specification, tests/vad_ref.py restates it in numpy, and the
kernels are checked against that: decisions bit for bit, normalised values within the fp64 summation bound.

    v = energy_vad(mfcc, lengths)                          # Vad: .mask [B, T] uint8, .counts [B] int32, .threshold [B] float64
    y = sliding_cmvn(mfcc, lengths, cmn_window=300, center=True)          # [B, T, C], zeros past every length
    z, n = select_voiced(mfcc, v.mask, lengths)                           # the voiced rows first, zeros behind; n [B] int32

    prep = VadCmvn()                                       # the recipe's settings: VAD, CMVN over 3 s, voiced frames only
    p = prep(mfcc, lengths)                                # Prepared: .feats [B, T, C], .lengths (host list), .mask
    xv = model.extract_x_vec(p.feats, p.lengths)

    d = Diarizer(model, scorer, frontend=VadCmvn(), threshold=0.0)        # windows inside the speech runs only

Everything stays on the device but `Prepared.lengths`, which the extractor's ragged calls take from the host: the one small
copy.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, ptr as _ptr, stream as _stream

__all__ = ["energy_vad", "sliding_cmvn", "select_voiced", "VadCmvn", "Vad", "Prepared", "speech_runs", "run_windows", "LANES",
           "MAX_CHANNELS", "MAX_WINDOW", "TILE_MAX", "TILE_MIN", "GROUP_MIN", "LDS_BYTES", "VAD_DEFAULTS", "CMVN_DEFAULTS"]

# include/xvec_vad.h: XVEC_VAD_LANES, XVEC_VAD_MAX_CHANNELS, XVEC_CMVN_MAX_WINDOW, XVEC_CMVN_TILE_MAX / _MIN,
# XVEC_CMVN_GROUP_MIN, XVEC_CMVN_LDS_BYTES
LANES, MAX_CHANNELS, MAX_WINDOW, TILE_MAX, TILE_MIN, GROUP_MIN, LDS_BYTES = 256, 1024, 1900, 256, 16, 8, 61440
# the defaults of compute-vad-decision and apply-cmvn-sliding
VAD_DEFAULTS = dict(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6, energy_col=0)
CMVN_DEFAULTS = dict(cmn_window=600, min_window=100, center=False, norm_vars=False)

_check = checker(_hip.lib.xvec_vad_last_error)


class Vad(NamedTuple):
    mask: torch.Tensor          # [B, T] uint8: 1 = voiced; 0 at or past the length
    counts: torch.Tensor        # [B] int32: the voiced frames
    threshold: torch.Tensor     # [B] float64: the energy threshold of every utterance


class Prepared(NamedTuple):
    feats: torch.Tensor         # [B, T, C] float32: the (voiced) rows first, zeros behind
    lengths: list               # HOST: the rows of every utterance
    mask: torch.Tensor          # [B, T] uint8: the decisions, in the input's frames


def _vad_options(opts) -> _hip.VadOptions:
    unknown = set(opts) - set(VAD_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown VAD option(s) {sorted(unknown)}: expected {sorted(VAD_DEFAULTS)}")
    o = {**VAD_DEFAULTS, **opts}
    return _hip.VadOptions(float(o["energy_threshold"]), float(o["energy_mean_scale"]), float(o["proportion_threshold"]),
                           int(o["frames_context"]), int(o["energy_col"]))


def _cmvn_options(opts) -> _hip.CmvnOptions:
    unknown = set(opts) - set(CMVN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown CMVN option(s) {sorted(unknown)}: expected {sorted(CMVN_DEFAULTS)}")
    o = {**CMVN_DEFAULTS, **opts}
    return _hip.CmvnOptions(int(o["cmn_window"]), int(o["min_window"]), int(bool(o["center"])), int(bool(o["norm_vars"])))


def _feats(x, what) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): the features must be a device tensor")
    if x.dim() != 3 or x.dtype != torch.float32 or min(x.shape) < 1:
        raise ValueError(f"{what}: expected float32 features [B, T, C], none of them empty, got {x.dtype} {tuple(x.shape)}")
    x = x.detach()
    # the library takes a row and an utterance stride: a view that only pads rows or utterances needs no copy
    ok = x.stride(2) == 1 and x.stride(1) >= x.shape[2] and x.stride(0) >= (x.shape[1] - 1) * x.stride(1) + x.shape[2]
    return x if ok else x.contiguous()


def _lengths(lengths, x) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    t = torch.as_tensor(lengths).detach().to(device=x.device, dtype=torch.int32).contiguous()
    if t.dim() != 1 or t.shape[0] != x.shape[0]:
        raise ValueError(f"lengths has shape {tuple(t.shape)} for a batch of {x.shape[0]}")
    return t


def _workspace(x, cached=None) -> torch.Tensor:
    return byte_workspace(int(_hip.lib.xvec_vad_workspace_bytes(x.shape[0], x.shape[1])), x.device, cached)


def energy_vad(feats, lengths=None, **opts) -> Vad:
    """Energy-based decisions on the device features [B, T, C] (`lengths`: valid frames of each, host or device): a frame is
    voiced when at least `proportion_threshold` of the frames within `frames_context` of it have an energy (column
    `energy_col`) above `energy_threshold + energy_mean_scale *` the utterance's mean energy."""
    opt = _vad_options(opts)
    x = _feats(feats, "energy_vad")
    B, T, C = (int(v) for v in x.shape)
    lens = _lengths(lengths, x)
    mask = torch.empty((B, T), dtype=torch.uint8, device=x.device)
    counts = torch.empty(B, dtype=torch.int32, device=x.device)
    thr = torch.empty(B, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(_hip.lib.xvec_vad_energy(x.data_ptr(), B, T, C, x.stride(1), x.stride(0), _ptr(lens), opt, mask.data_ptr(), T,
                                        counts.data_ptr(), thr.data_ptr(), _stream(x.device)))
    return Vad(mask, counts, thr)


def _normalise(x, lens, cmvn, mask, workspace=None):
    B, T, C = (int(v) for v in x.shape)
    y = torch.empty((B, T, C), dtype=torch.float32, device=x.device)
    new_len = torch.empty(B, dtype=torch.int32, device=x.device)
    ws = _workspace(x, workspace)
    with torch.cuda.device(x.device):
        _check(_hip.lib.xvec_cmvn_sliding(x.data_ptr(), B, T, C, x.stride(1), x.stride(0), _ptr(lens), cmvn, _ptr(mask),
                                          0 if mask is None else mask.stride(0), y.data_ptr(), C, T * C, new_len.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream(x.device)))
    return y, new_len


def sliding_cmvn(feats, lengths=None, **opts) -> torch.Tensor:
    """The features minus the mean over a window of `cmn_window` frames around (`center`) or before every frame -- at least
    `min_window` frames where the utterance has them -- and with `norm_vars` over the window's standard deviation.  [B, T, C]
    like the input, zeros at and past every length."""
    opt = _cmvn_options(opts)
    x = _feats(feats, "sliding_cmvn")
    return _normalise(x, _lengths(lengths, x), opt, None)[0]


def _mask(mask, x, what) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or mask.device != x.device or mask.shape != x.shape[:2]:
        raise ValueError(f"{what}: the mask must be a [B, T] tensor on the features' device")
    m = mask.detach()
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    if m.dtype != torch.uint8:
        raise ValueError(f"{what}: the mask must be uint8 or bool, got {m.dtype}")
    return m if m.stride(1) == 1 and m.stride(0) >= m.shape[1] else m.contiguous()


def select_voiced(feats, mask, lengths=None):
    """(rows, new_lengths): every utterance's voiced rows in order, bit-exact copies, zeros behind them; new_lengths [B] int32
    on the device."""
    x = _feats(feats, "select_voiced")
    return _normalise(x, _lengths(lengths, x), None, _mask(mask, x, "select_voiced"))


class VadCmvn:
    """The recipe's front end behind the MFCCs: energy VAD, sliding CMVN and (with `select`) the voiced frames only, two
    launches.  `vad`: the VAD options, or None for the normalisation alone -- the call then returns a bare tensor, which is
    what `stream_x_vectors(prepare=...)` takes.  `cmn_window=None` leaves the rows as they are (VAD and selection only)."""

    def __init__(self, cmn_window=300, center=True, norm_vars=False, min_window=100,
                 vad=dict(energy_threshold=5.5, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.12), select=True):
        self.cmvn = None if cmn_window is None else _cmvn_options(dict(cmn_window=cmn_window, center=center, norm_vars=norm_vars,
                                                                       min_window=min_window))
        self.vad = None if vad is None else _vad_options(dict(vad))
        if self.vad is None and self.cmvn is None:
            raise ValueError("VadCmvn: neither a VAD nor a normalisation")
        self.select = bool(select)
        self._ws = None

    def with_select(self, select) -> "VadCmvn":
        """The same settings with another `select`."""
        other = VadCmvn.__new__(VadCmvn)
        other.cmvn, other.vad, other.select, other._ws = self.cmvn, self.vad, bool(select), None
        return other

    def __call__(self, feats, lengths=None):
        x = _feats(feats, "VadCmvn")
        lens = _lengths(lengths, x)
        if self.vad is None:
            return _normalise(x, lens, self.cmvn, None)[0]
        B, T, C = (int(v) for v in x.shape)
        dev = x.device
        mask = torch.empty((B, T), dtype=torch.uint8, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        new_len = torch.empty(B, dtype=torch.int32, device=dev)
        y = torch.empty((B, T, C), dtype=torch.float32, device=dev)
        self._ws = _workspace(x, self._ws)
        with torch.cuda.device(dev):
            _check(_hip.lib.xvec_vad_cmvn(x.data_ptr(), B, T, C, x.stride(1), x.stride(0), _ptr(lens), self.vad, self.cmvn,
                                          int(self.select), mask.data_ptr(), T, counts.data_ptr(), None, y.data_ptr(), C, T * C,
                                          new_len.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _stream(dev)))
        return Prepared(y, new_len.cpu().tolist(), mask)


def speech_runs(mask, lengths=None, max_gap=0, min_len=15) -> np.ndarray:
    """int32 [n, 3] rows (utt, start, len): the runs of voiced frames of every utterance of `mask` [B, T] (below `lengths`),
    ordered by utterance, then start.  Gaps of at most `max_gap` frames between two runs are closed first; then runs shorter
    than `min_len` are dropped (15: what a window of the extractor needs).  Host arithmetic on the copied mask."""
    m = np.asarray(mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask)
    if m.ndim != 2:
        raise ValueError(f"speech_runs: expected a mask [B, T], got shape {m.shape}")
    B, T = m.shape
    if lengths is None:
        lens = [T] * B
    else:
        lens = [int(v) for v in (lengths.detach().cpu().tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(lens) != B:
            raise ValueError(f"speech_runs: lengths has {len(lens)} entries for a batch of {B}")
    max_gap, min_len = int(max_gap), int(min_len)
    rows = []
    for u in range(B):
        v = np.concatenate([[0], (m[u, :max(0, min(lens[u], T))] != 0).astype(np.int8), [0]])
        edges = np.flatnonzero(np.diff(v))                       # rises and falls, alternating
        runs = []
        for a, b in zip(edges[0::2].tolist(), edges[1::2].tolist()):
            if runs and a - runs[-1][1] <= max_gap:
                runs[-1][1] = b
            else:
                runs.append([a, b])
        rows += [(u, a, b - a) for a, b in runs if b - a >= min_len]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def run_windows(runs, win, hop, min_tail=None) -> np.ndarray:
    """int32 [n, 3] rows (utt, start, len): `sliding_windows` inside every run of `runs` [m, 3] (utt, start, len), the starts in
    the recording's frames; ordered as the runs are."""
    from .model import sliding_windows
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 3)
    if not len(runs):
        return np.zeros((0, 3), dtype=np.int32)
    w = sliding_windows(runs[:, 2].tolist(), win, hop, min_tail).astype(np.int64)
    out = np.stack([runs[w[:, 0], 0], runs[w[:, 0], 1] + w[:, 1], w[:, 2]], axis=1)
    return out.astype(np.int32).reshape(-1, 3)
