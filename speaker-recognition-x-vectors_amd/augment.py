"""Waveform augmentation on the GPU: the stage in front of the MFCC front end (reference dataset.py:185-396).

The reference augments one utterance at a time on DataLoader workers: MUSAN noise added at a drawn SNR (`music`, `speech`,
`noise`), a simulated room impulse response (`rir`), and then, for EVERY sample, augmented or not, the scaling
`(x - min) / max(x - min)` (dataset.py:217-219) before `mfcc`.  Here the clips and the impulse responses live on the device,
the host only draws (which clip, which start, which SNR: `AugmentPlan.draw` makes the reference's draws in the reference's
order), and three HIP stages do the arithmetic on a whole batch (include/xvec_augment.h):

    aug = WaveAugmenter(pool, pool_len, rirs, rir_len, device="cuda:0")   # pool int16 or float32 [R, m_max]
    plan = AugmentPlan.draw(kinds, n, music_rows, speech_rows, noise_rows, n_rirs, pool_len=pool_len)
    feats = fe(aug(waves, plan))                    # mix -> reverb -> normalize -> MfccFrontEnd
    feats = fe(aug.normalize(waves))                # no augmentation: what the reference feeds its model at test time

A reference-faithful front end needs at least `normalize`.  Not covered: reading files and resampling (resampy is not
installed where this was built, so that part of the reference's path is unpinned): the pool holds clips that already have
the utterances' sampling rate.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import random as _random

import numpy as np
import torch

from . import hip as _hip
from ._device import checker, require_device, sized_workspace, stream as _stream

__all__ = ["WaveAugmenter", "AugmentPlan", "KINDS"]

KINDS = ("none", "music", "speech", "noise", "rir")

OP_DTYPE = np.dtype([("utt", "<i4"), ("offset", "<i4"), ("length", "<i4"), ("first_src", "<i4"), ("n_src", "<i4"),
                     ("reserved", "<i4"), ("snr_ratio", "<f8")])                 # xvec_aug_op
SRC_DTYPE = np.dtype([("row", "<i4"), ("start", "<i4")])                         # xvec_aug_src

_check = checker(_hip.lib.xvec_aug_last_error)


class AugmentPlan:
    """The draws of one batch: `ops` (host, xvec_aug_op records sorted by utterance), `srcs` (xvec_aug_src records) and
    `rir_index` (int32 [B], -1 = no reverberation); `snr_db` keeps the drawn SNR of every op for logging."""

    def __init__(self, ops, srcs, rir_index, snr_db=None):
        self.ops = np.ascontiguousarray(ops, dtype=OP_DTYPE)
        self.srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
        self.rir_index = np.ascontiguousarray(rir_index, dtype=np.int32)
        self.snr_db = None if snr_db is None else np.asarray(snr_db, dtype=np.int64)
        if self.ops.ndim != 1 or self.srcs.ndim != 1 or self.rir_index.ndim != 1:
            raise ValueError("AugmentPlan: ops, srcs and rir_index must be vectors")
        self._dev = {}

    def __len__(self):
        return int(self.rir_index.shape[0])

    @classmethod
    def draw(cls, kinds, n, music_rows, speech_rows, noise_rows, n_rirs, samplerate=16000, rng=_random,
             noise_offsets="reference", *, pool_len):
        """The reference's draws for one kind per utterance ('none' | 'music' | 'speech' | 'noise' | 'rir'), made on `rng`
        (`choice` and `randint`, as the reference calls its `random`) in the reference's order.  `n` is the utterance
        length (the reference's 3 s crop), `*_rows` the pool rows of each MUSAN kind in the order the reference lists its
        files, `pool_len` the clip lengths of the pool (a clip longer than what is needed is cropped at a drawn start, a
        shorter one is zero-padded and draws nothing, as cut_to_sec).

          music   one clip, SNR randint(5, 15), one op over the whole row
          speech  the sum of 1 + randint(2, 6) clips, SNR randint(13, 20), one op over the whole row
          noise   three clips of `samplerate` samples, SNR randint(0, 15) each: three ops of that length
          rir     one of `n_rirs` responses; no op

        noise_offsets="reference" puts the three noise ops at samples 0, 1, 2: the reference indexes `sample[i:i + rate]`
        with i = 0, 1, 2 (dataset.py:359-364), so its one-second clips overlap almost entirely.  "seconds" puts them at
        0, samplerate, 2 * samplerate, which is what its docstring describes: a DEVIATION from what it computes."""
        if noise_offsets not in ("reference", "seconds"):
            raise ValueError("noise_offsets: 'reference' or 'seconds'")
        pool_len = np.asarray(pool_len).astype(np.int64)
        ops, srcs, snrs, rir_index = [], [], [], []

        def clip(rows, length):
            row = int(rng.choice(list(rows)))
            have = int(pool_len[row])
            start = 0 if have < length else int(rng.randint(0, have - length))
            srcs.append((row, start))

        def op(utt, offset, length, first, lo, hi):
            snr = int(rng.randint(lo, hi))
            snrs.append(snr)
            ops.append((utt, offset, length, first, len(srcs) - first, 0, 10 ** (snr / 10)))

        for utt, kind in enumerate(kinds):
            rir = -1
            first = len(srcs)
            if kind == "music":
                clip(music_rows, n)
                op(utt, 0, n, first, 5, 15)
            elif kind == "speech":
                clip(speech_rows, n)
                for _ in range(int(rng.randint(2, 6))):
                    clip(speech_rows, n)
                op(utt, 0, n, first, 13, 20)
            elif kind == "noise":
                if n < 2 * (samplerate if noise_offsets == "seconds" else 1) + samplerate:
                    raise ValueError(f"noise: three {samplerate}-sample clips do not fit an utterance of {n} samples")
                for i in range(3):
                    first = len(srcs)
                    clip(noise_rows, samplerate)
                    op(utt, i * samplerate if noise_offsets == "seconds" else i, samplerate, first, 0, 15)
            elif kind == "rir":
                rir = int(rng.choice(range(n_rirs)))
            elif kind != "none":
                raise ValueError(f"unknown augmentation kind {kind!r}: one of {KINDS}")
            rir_index.append(rir)
        return cls(np.array(ops, dtype=OP_DTYPE), np.array(srcs, dtype=SRC_DTYPE), rir_index, snrs)

    def on(self, device):
        """(srcs, rir_index) on `device`, copied once per device; the ops stay on the host (the library checks them there)."""
        key = str(device)
        if key not in self._dev:
            srcs = self.srcs if len(self.srcs) else np.zeros(1, dtype=SRC_DTYPE)       # never a null pointer
            self._dev[key] = (torch.from_numpy(srcs.view(np.int32).copy()).to(device),
                              torch.from_numpy(self.rir_index).to(device))
        return self._dev[key]


def _pool(a, lens, what, dtypes, device):
    t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected a [rows, samples] array")
    if t.dtype not in dtypes:
        t = t.to(dtypes[0])
    lens = torch.as_tensor(np.asarray(lens, dtype=np.int64) if not isinstance(lens, torch.Tensor) else lens)
    if lens.dim() != 1 or lens.numel() != t.shape[0]:
        raise ValueError(f"{what}: one length per row")
    if int(lens.min()) < 0 or int(lens.max()) > t.shape[1]:
        raise ValueError(f"{what}: a length lies outside 0 .. {t.shape[1]}")
    return t.to(device).contiguous(), lens.to(device=device, dtype=torch.int32).contiguous()


class WaveAugmenter:
    """Holds the clip pool (int16 or float32 [R, m_max] with `pool_len` [R]) and the impulse responses (float32
    [n_rirs, l_max] with `rir_len`) on `device`, and a byte workspace that grows to the largest batch seen.  Either pool
    may be None when its stage is not used.  Every method returns a new float32 [B, n] tensor on the device unless `inplace` is set."""

    def __init__(self, pool=None, pool_len=None, rirs=None, rir_len=None, device="cuda:0"):
        self.device = require_device(device, "waveform augmentation")
        self.pool = self.pool_len = self.rirs = self.rir_len = None
        if pool is not None:
            self.pool, self.pool_len = _pool(pool, pool_len, "pool", (torch.float32, torch.int16), self.device)
        if rirs is not None:
            self.rirs, self.rir_len = _pool(rirs, rir_len, "rirs", (torch.float32,), self.device)
        self._ws = None
        self._status = torch.zeros(2, dtype=torch.int64, device=self.device)       # xvec_aug_status
        self.last_gains = None      # fp64 [n_ops] of the last mix, on the device

    # ------------------------------------------------------------------ plumbing
    def _waves(self, waves, inplace=False) -> torch.Tensor:
        if not isinstance(waves, torch.Tensor) or not waves.is_cuda:
            raise RuntimeError("waveform augmentation runs on a HIP device only (no CPU path): pass a device tensor")
        if waves.dim() != 2 or waves.shape[0] < 1 or waves.shape[1] < 1:
            raise ValueError("expected waveforms [B, n]")
        if inplace:      # rows may be strided (a view into a larger buffer): the row stride is passed on
            if waves.dtype != torch.float32 or waves.device != self.device or waves.stride(1) != 1 or \
                    (waves.shape[0] > 1 and waves.stride(0) < waves.shape[1]):
                raise ValueError("inplace: float32 rows of unit stride on the augmenter's device")
            return waves
        return waves.detach().to(device=self.device, dtype=torch.float32, copy=True).contiguous()

    def _workspace(self, need: int) -> torch.Tensor:
        refusal = lambda: ValueError("waveform augmentation: batch or length outside the supported range")
        self._ws = sized_workspace(need, refusal, self.device, self._ws)
        return self._ws

    def status(self):
        """(sources skipped by the last mix, utterances whose rir was out of range in the last reverb); synchronises."""
        a, b = self._status.cpu().tolist()
        return int(a), int(b)

    # ------------------------------------------------------------------ stages (in place on a private copy)
    def _mix(self, out, plan):
        if self.pool is None:
            raise RuntimeError("WaveAugmenter.mix: no clip pool was given")
        B, n = out.shape
        n_ops = len(plan.ops)
        srcs, _ = plan.on(self.device)
        gains = torch.empty(max(n_ops, 1), dtype=torch.float64, device=self.device)
        ws = self._workspace(int(_hip.lib.xvec_aug_mix_workspace_bytes(B, n, n_ops)))
        dtype = _hip.AUG_POOL_I16 if self.pool.dtype == torch.int16 else _hip.AUG_POOL_F32
        with torch.cuda.device(self.device):
            _check(_hip.lib.xvec_aug_mix(out.data_ptr(), max(out.stride(0), n), B, n, self.pool.data_ptr(), dtype,
                                         self.pool.shape[0], self.pool.shape[1], self.pool_len.data_ptr(),
                                         plan.ops.ctypes.data_as(C.c_void_p), n_ops, srcs.data_ptr(), len(plan.srcs),
                                         gains.data_ptr(), self._status.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream(self.device)))
        self.last_gains = gains[:n_ops]
        return out

    def _reverb(self, out, rir_index):
        if self.rirs is None:
            raise RuntimeError("WaveAugmenter.reverb: no impulse responses were given")
        B, n = out.shape
        idx = torch.as_tensor(rir_index).to(device=self.device, dtype=torch.int32).contiguous()
        if idx.dim() != 1 or idx.numel() != B:
            raise ValueError("reverb: one rir index per utterance (-1 = none)")
        ws = self._workspace(int(_hip.lib.xvec_aug_reverb_workspace_bytes(B, n, self.rirs.shape[1])))
        with torch.cuda.device(self.device):
            _check(_hip.lib.xvec_aug_reverb(out.data_ptr(), max(out.stride(0), n), B, n, self.rirs.data_ptr(),
                                            self.rirs.shape[0], self.rirs.shape[1], self.rir_len.data_ptr(), idx.data_ptr(),
                                            self._status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(self.device)))
        return out

    def _normalize(self, out):
        B, n = out.shape
        with torch.cuda.device(self.device):
            _check(_hip.lib.xvec_aug_normalize(out.data_ptr(), max(out.stride(0), n), B, n, _stream(self.device)))
        return out

    def mix(self, waves, plan: AugmentPlan, inplace=False) -> torch.Tensor:
        """The plan's ops (add_with_certain_snr); rows without ops come back unchanged.  `last_gains` keeps the factors.
        `inplace` (here and below) works on `waves` itself: float32, rows of unit stride, any row stride >= n."""
        out = self._waves(waves, inplace)
        if len(plan) != out.shape[0]:
            raise ValueError(f"mix: a plan for {len(plan)} utterances and a batch of {out.shape[0]}")
        return self._mix(out, plan)

    def reverb(self, waves, rir_index, inplace=False) -> torch.Tensor:
        """x + (x * h)[:n] * (max|x| / max|x * h|) with h = rirs[rir_index[b]]; -1 leaves a row as it is."""
        return self._reverb(self._waves(waves, inplace), rir_index)

    def normalize(self, waves, inplace=False) -> torch.Tensor:
        """(x - min) / (max - min) per row: what the reference applies to every sample before `mfcc`."""
        return self._normalize(self._waves(waves, inplace))

    def __call__(self, waves, plan: AugmentPlan = None) -> torch.Tensor:
        """mix -> reverb -> normalize, each stage only if the plan asks for it (normalize always): float32 [B, n] ready for
        MfccFrontEnd."""
        out = self._waves(waves)
        if plan is not None:
            if len(plan) != out.shape[0]:
                raise ValueError(f"a plan for {len(plan)} utterances and a batch of {out.shape[0]}")
            if len(plan.ops):
                self._mix(out, plan)
            if (plan.rir_index >= 0).any():
                self._reverb(out, plan.on(self.device)[1])
        return self._normalize(out)
