"""DER on the GPU: the diarization error rate of hypothesis turns against reference turns (include/xvec_der.h).

Miss, false alarm and speaker confusion over integer ticks, with overlapped speech on both sides, a no-score collar and the
one-to-one speaker mapping that maximises the matched time, per recording and pooled.  Everything is integer arithmetic: the
counts are exact.  The definition follows NIST md-eval's; the header's text is the specification and tests/der_ref.py its numpy
restatement.  md-eval, dscore and pyannote.metrics are not dependencies and parity with them is unpinned.

    ref, rec_names, spk_names = read_rttm("ref.rttm")           # host: [m, 4] (rec, start, end, spk) like turns()
    res = d.diarize(mfcc_batch, lengths=lengths)                # a Diarizer (diarize.py)
    out = der(ref, res.turns, lengths, collar=25)
    out.der, out.overall, out.miss, out.fa, out.conf, out.mapping       # device tensors

There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, i64_ptr, ptr, require_device, sized_workspace, stream as _stream

__all__ = ["der", "assign", "read_rttm", "workspace_bytes", "DerResult", "MAX_SPEAKERS", "CHUNK_TICKS", "WAVE_ROWS", "THREADS"]

# include/xvec_der.h: the most speakers of a side in one recording, the ticks a block of the counting pass owns, the rows of
# 64 ticks a wave of it walks, the threads of a block
MAX_SPEAKERS, CHUNK_TICKS, WAVE_ROWS, THREADS = 64, 4096, 16, 256

_check = checker(_hip.lib.xvec_der_last_error)
_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1


class DerResult(NamedTuple):
    scored: torch.Tensor          # [n_rec] int64: scored ticks
    total: torch.Tensor           # [n_rec] int64: reference speaker time
    miss: torch.Tensor            # [n_rec] int64
    fa: torch.Tensor              # [n_rec] int64
    conf: torch.Tensor            # [n_rec] int64
    der: torch.Tensor             # [n_rec] float64, NaN for a recording without scored reference speech
    overall: torch.Tensor         # [] float64: the summed errors over the summed totals
    mapping: torch.Tensor         # [n_rec, 64] int32: the hypothesis speaker of every reference speaker, or -1
    ignored: tuple                # (reference, hypothesis) turns that were invalid: host integers
    cooccurrence: Optional[torch.Tensor] = None      # [n_rec, 64, 64] int64 with return_cooccurrence=True


def read_rttm(file, frame_shift=0.01, names=None):
    """(turns int64 [m, 4] of (rec, start, end, spk), recording names, speaker names per recording) of the SPEAKER lines of
    an RTTM file (a path or an open text file): the inverse of diarize.write_rttm.  start = int(rint(onset / frame_shift)),
    end likewise from onset + dur.  Recordings are numbered by `names`, or in the order of first appearance; speakers per
    recording in the order of first appearance.  A 65th speaker in one recording raises ValueError."""
    if hasattr(file, "read"):
        lines = file.read().splitlines()
    else:
        with open(file) as f:
            lines = f.read().splitlines()
    rec_names = list(names) if names is not None else []
    rec_of = {n: k for k, n in enumerate(rec_names)}
    spk_of = [dict() for _ in rec_names]
    out = []
    for no, line in enumerate(lines, 1):
        f = line.split()
        if not f or f[0] != "SPEAKER":
            continue
        if len(f) < 8:
            raise ValueError(f"read_rttm: line {no} has {len(f)} fields, a SPEAKER line has 8 or more")
        name, onset, dur, spk = f[1], float(f[3]), float(f[4]), f[7]
        if name not in rec_of:
            if names is not None:
                raise ValueError(f"read_rttm: line {no} names the recording {name!r}, which is not among `names`")
            rec_of[name] = len(rec_names)
            rec_names.append(name)
            spk_of.append({})
        r = rec_of[name]
        if spk not in spk_of[r]:
            if len(spk_of[r]) == MAX_SPEAKERS:
                raise ValueError(f"read_rttm: line {no}: {spk!r} is speaker {MAX_SPEAKERS + 1} of {name!r}, {MAX_SPEAKERS} are the most")
            spk_of[r][spk] = len(spk_of[r])
        out.append([r, int(np.rint(onset / frame_shift)), int(np.rint((onset + dur) / frame_shift)), spk_of[r][spk]])
    return np.asarray(out, dtype=np.int64).reshape(-1, 4), rec_names, [list(d) for d in spk_of]


def _turns(t, device, what) -> Optional[torch.Tensor]:
    """A turn list as the library reads it: int32 [m, 4] on the device, values outside int32 clamped to its ends (such a
    value is outside every recording and every speaker range either way); None for an empty list."""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"der: {what} turns must be integers, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(-1, 4) if a.size == 0 else a, dtype=np.int64))
    elif t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"der: {what} turns must be integers, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError(f"der: {what} turns must be [m, 4] rows of (rec, start, end, spk), got {tuple(t.shape)}")
    if t.shape[0] == 0:
        return None
    t = t.to(device)
    if t.dtype != torch.int32:
        t = t.to(torch.int64).clamp(_I32_MIN, _I32_MAX).to(torch.int32)
    return t.contiguous()


def _rec_start(rec_len) -> np.ndarray:
    n = np.asarray(rec_len.cpu().numpy() if isinstance(rec_len, torch.Tensor) else rec_len)
    if n.ndim != 1 or n.shape[0] < 1 or n.dtype.kind not in "iu" or (n < 1).any():
        raise ValueError("der: rec_len must be the ticks of every recording, integers of 1 or more")
    return np.concatenate([[0], np.cumsum(n.astype(np.int64))]).astype(np.int64)


def workspace_bytes(rec_len, m_ref=0, m_hyp=0) -> int:
    """Bytes of workspace `der` needs for recordings of these lengths (0: the arguments are refused)."""
    rs = _rec_start(rec_len)
    return int(_hip.lib.xvec_der_workspace_bytes(i64_ptr(rs), rs.shape[0] - 1, int(m_ref), int(m_hyp)))


def der(ref_turns, hyp_turns, rec_len, collar=0, skip_overlap=False, strict=True, return_cooccurrence=False, workspace=None,
        device="cuda:0") -> DerResult:
    """The diarization error rate of `hyp_turns` against `ref_turns`, both [m, 4] rows of (rec, start, end, spk) in ticks as
    diarize.turns() returns them (numpy or torch, any integer dtype; device tensors are used where they are), over recordings
    of `rec_len` ticks each.  `collar`: ticks left unscored on either side of every reference boundary; `skip_overlap`: leave
    ticks with two or more reference speakers unscored.  A turn with a recording or speaker out of range or without a tick is
    ignored and counted (`ignored`, the one thing read back); `strict=True` raises if there is one."""
    for t in (ref_turns, hyp_turns):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            device = t.device
            break
    dev = require_device(device, "der")
    ref, hyp = _turns(ref_turns, dev, "reference"), _turns(hyp_turns, dev, "hypothesis")
    rs = _rec_start(rec_len)
    n_rec = rs.shape[0] - 1
    m_ref, m_hyp = (0 if ref is None else int(ref.shape[0])), (0 if hyp is None else int(hyp.shape[0]))
    rs_p = i64_ptr(rs)
    refusal = lambda: ValueError(f"der: {int(rs[-1])} ticks in {n_rec} recordings: the total must stay below 2^31")
    ws = sized_workspace(_hip.lib.xvec_der_workspace_bytes(rs_p, n_rec, m_ref, m_hyp), refusal, dev, workspace)
    if int(collar) < 0:
        raise ValueError(f"der: collar = {collar} must not be negative")
    counts = torch.empty((n_rec, 5), dtype=torch.int64, device=dev)
    mapping = torch.empty((n_rec, MAX_SPEAKERS), dtype=torch.int32, device=dev)
    rate = torch.empty(n_rec + 1, dtype=torch.float64, device=dev)
    ign = torch.empty(2, dtype=torch.int64, device=dev)
    cooc = torch.empty((n_rec, MAX_SPEAKERS, MAX_SPEAKERS), dtype=torch.int64, device=dev) if return_cooccurrence else None
    with torch.cuda.device(dev):
        _check(_hip.lib.xvec_der_score(ptr(ref), m_ref, ptr(hyp), m_hyp, rs_p, n_rec, int(collar), 1 if skip_overlap else 0,
                                       counts.data_ptr(), mapping.data_ptr(), rate.data_ptr(), ign.data_ptr(), ptr(cooc),
                                       ws.data_ptr(), ws.numel(), _stream(dev)))
    ignored = tuple(int(v) for v in ign.cpu().tolist())          # the call's one copy to the host
    if strict and any(ignored):
        raise ValueError(f"der: {ignored[0]} reference and {ignored[1]} hypothesis turns are invalid (a recording outside "
                         f"0 .. {n_rec - 1}, a speaker outside 0 .. {MAX_SPEAKERS - 1}, or end <= start); strict=False counts them instead")
    return DerResult(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], counts[:, 4], rate[:n_rec], rate[n_rec], mapping,
                     ignored, cooc)


def assign(cooc):
    """(mapping [n, 64] int32, correct [n] int64) of a device batch of 64 x 64 co-occurrence matrices `cooc` [n, 64, 64] (or
    one [64, 64]) with entries in 0 .. 2^31 - 1: the partial one-to-one map from rows to columns with the largest sum; -1
    where a row has no partner with a positive entry."""
    if not isinstance(cooc, torch.Tensor) or not cooc.is_cuda:
        raise RuntimeError("assign runs on a HIP device only (no CPU path): the matrices must be a device tensor")
    single = cooc.dim() == 2
    c = cooc.unsqueeze(0) if single else cooc
    if c.dim() != 3 or c.shape[0] < 1 or tuple(c.shape[1:]) != (MAX_SPEAKERS, MAX_SPEAKERS) or c.is_floating_point():
        raise ValueError(f"assign: expected integer [n, {MAX_SPEAKERS}, {MAX_SPEAKERS}] matrices, got {tuple(cooc.shape)} {cooc.dtype}")
    c = c.to(torch.int64).contiguous()
    dev, n = c.device, int(c.shape[0])
    mapping = torch.empty((n, MAX_SPEAKERS), dtype=torch.int32, device=dev)
    correct = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _check(_hip.lib.xvec_der_assign(c.data_ptr(), n, mapping.data_ptr(), correct.data_ptr(), _stream(dev)))
    return (mapping[0], correct[0]) if single else (mapping, correct)
