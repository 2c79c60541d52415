"""Waveform resampling on the GPU: resampy's band-limited sinc interpolation at any ratio (include/xvec_resample.h).

The first arithmetic stage of the reference's Dataset.__getitem__ (dataset.py:125-130: wavfile.read -> resampy.resample ->
cut_to_sec -> augment_data -> min/max -> mfcc); the stages behind it are `augment.WaveAugmenter` and `frontend.MfccFrontEnd`.
The reference resamples every file and every MUSAN clip, also at equal rates, where the signal still passes through the
filter's low-pass: a `Resampler(16000, 16000)` is NOT the identity, as the package is not.

    y = resample(x, sr_orig, 16000)                                    # numpy in, numpy out: the call at dataset.py:126

    rs = Resampler(8000, 16000, device="cuda:0")                       # device tensors throughout
    waves16k = rs(pcm8k)                                               # [B, n] int16 / float32 -> [B, rs.num_out(n)] float32
    out, out_lens = rs(padded, lens)                                   # ragged rows: zeros past out_lens[b]
    fast_slow, lens = speed_perturb(waves, [0.9, 1.0, 1.1])            # row b at ratio 1 / factors[b], one launch

Parity with resampy itself is UNPINNED (not installed where this was written): the arithmetic is resampy 0.3.0's, restated from
memory -- the filter tables below, `n_out = int(n * ratio)`, the truncated table step `int(ratio * 2 ** precision)` when
downsampling (512 / 3 -> 170: a 48 kHz -> 16 kHz sine comes out 2.7e-3 off the analytic one, as in the package at that
version), the left wing before the right, every fp64 operation rounded on its own.  tests/resample_ref.py holds the restatement
in numpy, and the kernel equals it bit for bit.  "kaiser_fast" is recalled with less confidence than "kaiser_best"; any
(half_window, precision) pair can be passed in place of a name.  There is no CPU path.
"""
from __future__ import annotations

import sys
import types

import numpy as np
import torch

from . import hip as _hip
from ._device import byte_workspace, checker, require_device, stream as _stream

__all__ = ["FILTERS", "sinc_window", "Resampler", "speed_perturb", "resample", "resample_rows", "tile_span", "TILE", "SPAN_MAX",
           "PRECISION_MAX"]

TILE = 256                # XVEC_RESAMPLE_TILE: consecutive outputs of one row a block owns
SPAN_MAX = 8192           # XVEC_RESAMPLE_SPAN_MAX: input samples of a tile staged in LDS; rows whose tiles need more read memory
PRECISION_MAX = 20        # XVEC_RESAMPLE_PRECISION_MAX
X_F32, X_I16 = 0, 1       # XVEC_RESAMPLE_X_*
OUT_F32, OUT_F64 = 0, 1   # XVEC_RESAMPLE_OUT_*
ACC_F32, ACC_F64 = 0, 1   # XVEC_RESAMPLE_ACC_*
LEN_I64, LEN_I32 = 0, 1   # XVEC_RESAMPLE_LEN_*

# resampy 0.3.0's precomputed filters, as sinc_window arguments (restated from memory; kaiser_fast with less confidence)
FILTERS = {
    "kaiser_best": dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492),
    "kaiser_fast": dict(num_zeros=16, precision=9, rolloff=0.85, beta=8.555504641634386),
}

_check = checker(_hip.lib.xvec_resample_last_error)
_ACC = {"float32": ACC_F32, "float64": ACC_F64}
_tables = {}


def sinc_window(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596) -> np.ndarray:
    """The right half of a Kaiser-windowed sinc low-pass, float64 [num_zeros * 2 ** precision + 1]: `num_zeros` zero crossings,
    2 ** precision entries between two of them, cut-off at `rolloff` of Nyquist.  resampy.filters.sinc_window with a Kaiser
    window of shape `beta`.  Host only."""
    num_zeros, precision = int(num_zeros), int(precision)
    if num_zeros < 1 or not 0 <= precision <= PRECISION_MAX or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"sinc_window: num_zeros >= 1, 0 <= precision <= {PRECISION_MAX}, 0 < rolloff <= 1 "
                         f"(got {num_zeros}, {precision}, {rolloff})")
    m = (2 ** precision) * num_zeros
    taper = np.kaiser(2 * m + 1, beta)[m:]
    return rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=m + 1, endpoint=True)) * taper


def _table(filter):
    """(half_window float64 ndarray, precision) of a filter name or of a (half_window, precision) pair."""
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise ValueError(f"unknown filter {filter!r}: one of {sorted(FILTERS)} or a (half_window, precision) pair")
        if filter not in _tables:
            _tables[filter] = (sinc_window(**FILTERS[filter]), FILTERS[filter]["precision"])
        return _tables[filter]
    win, precision = filter
    win = np.ascontiguousarray(win, dtype=np.float64)
    if win.ndim != 1 or not 0 <= int(precision) <= PRECISION_MAX or win.shape[0] < 2 ** int(precision) + 1:
        raise ValueError("filter: a 1-D half window of at least 2 ** precision + 1 entries and its precision")
    return win, int(precision)


def tile_span(ratio, filter="kaiser_best") -> int:
    """Input samples one tile of TILE outputs can touch at `ratio`; rows with tile_span <= SPAN_MAX are staged in LDS."""
    win, precision = _table(filter)
    span = int(_hip.lib.xvec_resample_tile_span(float(ratio), win.shape[0], precision))
    if span < 0:
        raise ValueError(f"ratio = {ratio}: not a ratio this filter can resample at")
    return span


def _num_out(n, ratio) -> int:
    v = int(_hip.lib.xvec_resample_out_len(int(n), float(ratio)))
    if v < 0:
        raise ValueError(f"ratio = {ratio} must be finite and positive (n = {n})")
    return v


def resample_rows(waves, ratios, lens=None, filter="kaiser_best", accumulate=None, out_dtype=torch.float32, out=None,
                  workspace=None, win=None):
    """The launch: `waves` [B, n] device tensor (int16 / float32, unit column stride), row b at ratio `ratios[b]` (one ratio
    serves all rows), `lens` [B] valid samples per row (device int32 / int64 tensor or a host sequence; None: n everywhere).
    Returns (out, out_lens): out [B, max(1, longest output)] of `out_dtype` (float32 / float64), zero past out_lens[b], and
    out_lens [B] (the dtype of `lens`, int64 by default) = int(lens[b] * ratios[b]).  `out`: a device matrix to write into
    (at least that many columns, any row stride); `win`: the filter's table already on the device."""
    if not isinstance(waves, torch.Tensor):
        raise TypeError("resample_rows: waves must be a device tensor (resample() takes numpy arrays)")
    device = require_device(waves.device, "resampling")
    if waves.dim() != 2 or waves.shape[0] < 1 or waves.shape[1] < 1:
        raise ValueError(f"resample_rows: expected [B, n] waveforms, got shape {tuple(waves.shape)}")
    if waves.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"resample_rows: samples must be int16 or float32, got {waves.dtype}")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"resample_rows: out_dtype must be float32 or float64, got {out_dtype}")
    B, n = int(waves.shape[0]), int(waves.shape[1])
    if waves.stride(1) != 1 or (B > 1 and waves.stride(0) < n):
        waves = waves.contiguous()
    if accumulate is None:                         # as the package: int16 and float32 input give a float32 running sum
        accumulate = "float32"
    if accumulate not in _ACC:
        raise ValueError(f"accumulate = {accumulate!r}: 'float32' or 'float64'")
    ratios = np.ascontiguousarray(np.atleast_1d(np.asarray(ratios, dtype=np.float64)))
    if ratios.ndim != 1 or ratios.shape[0] not in (1, B):
        raise ValueError(f"resample_rows: one ratio or one per row, got {ratios.shape} for {B} rows")
    table, precision = _table(filter)
    if win is None:
        win = torch.from_numpy(table).to(device)
    cols = max(1, max(_num_out(n, r) for r in ratios))
    if lens is None:
        lens_d, len_dtype = None, torch.int64
    else:
        lens_d = lens if isinstance(lens, torch.Tensor) else torch.as_tensor(np.asarray(lens, dtype=np.int64))
        if lens_d.dtype not in (torch.int32, torch.int64) or lens_d.shape != (B,):
            raise ValueError(f"resample_rows: lens must be [B] int32 / int64, got {tuple(lens_d.shape)} {lens_d.dtype}")
        lens_d = lens_d.to(device).contiguous()
        len_dtype = lens_d.dtype
    if out is None:
        out = torch.empty((B, cols), dtype=out_dtype, device=device)
    elif (not isinstance(out, torch.Tensor) or out.device != device or out.dtype != out_dtype or out.dim() != 2
          or out.shape[0] != B or out.shape[1] < cols or out.stride(1) != 1 or (B > 1 and out.stride(0) < out.shape[1])):
        raise ValueError(f"resample_rows: out must be a {out_dtype} device matrix [B, >= {cols}] with unit column stride")
    out_lens = torch.empty(B, dtype=len_dtype, device=device)
    ws = byte_workspace(int(_hip.lib.xvec_resample_workspace_bytes(B, ratios.shape[0])), device, workspace)
    with torch.cuda.device(device):
        _check(_hip.lib.xvec_resample(
            waves.data_ptr(), X_I16 if waves.dtype == torch.int16 else X_F32, waves.stride(0) if B > 1 else n, B, n,
            None if lens_d is None else lens_d.data_ptr(), LEN_I32 if len_dtype == torch.int32 else LEN_I64,
            ratios.ctypes.data_as(_hip.C.POINTER(_hip.C.c_double)), ratios.shape[0], win.data_ptr(), table.shape[0], precision,
            _ACC[accumulate], out.data_ptr(), OUT_F64 if out_dtype == torch.float64 else OUT_F32,
            out.stride(0) if B > 1 else out.shape[1], out.shape[1], out_lens.data_ptr(), ws.data_ptr(), ws.numel(),
            _stream(device)))
    return out, out_lens


class Resampler:
    """resampy.resample(x, sr_orig, sr_new, filter=...) along the last axis of a batch of device waveforms.

    `filter`: "kaiser_best", "kaiser_fast" or a (half_window, precision) pair; `accumulate`: "float32" (the package's
    behaviour for int16 and float32 input, and the default: the running sum is rounded to float32 after every tap) or
    "float64"; `out_dtype`: torch.float32 or torch.float64."""

    def __init__(self, sr_orig, sr_new, filter="kaiser_best", accumulate=None, out_dtype=torch.float32, device="cuda:0"):
        if not (sr_orig > 0 and sr_new > 0):
            raise ValueError(f"Resampler: sample rates must be positive, got {sr_orig} -> {sr_new}")
        self.sr_orig, self.sr_new = sr_orig, sr_new
        self.ratio = float(sr_new) / sr_orig
        self.filter = filter
        self.table, self.precision = _table(filter)
        tile_span(self.ratio, (self.table, self.precision))       # raises for a ratio below 1 / 2 ** precision
        self.accumulate = accumulate
        self.out_dtype = out_dtype
        self.device = str(device)
        self._win = None

    def num_out(self, n) -> int:
        """int(n * ratio): the samples `n` input samples become."""
        return _num_out(n, self.ratio)

    def _device_table(self, device):
        if self._win is None or self._win.device != device:
            self._win = torch.from_numpy(self.table).to(device)
        return self._win

    def __call__(self, waves, lens=None, out=None, workspace=None):
        """`waves` [B, n] (or [n]) device tensor, int16 or float32 -> [B, num_out(n)] (or [num_out(n)]).  With `lens` [B]
        (valid samples per row): (out [B, max(1, num_out(n))] with zeros past out_lens[b], out_lens [B])."""
        device = require_device(self.device, "resampling")
        if not isinstance(waves, torch.Tensor):
            raise TypeError("Resampler: waves must be a device tensor (resample() takes numpy arrays)")
        require_device(waves.device, "resampling")
        one = waves.dim() == 1
        w = waves.unsqueeze(0) if one else waves
        if lens is None and w.dim() == 2 and self.num_out(w.shape[1]) < 1:
            raise ValueError(f"Input signal length={w.shape[1]} is too small to resample from {self.sr_orig}->{self.sr_new}")
        y, y_lens = resample_rows(w.to(device), [self.ratio], lens, (self.table, self.precision), self.accumulate,
                                  self.out_dtype, out, workspace, self._device_table(device))
        if lens is not None:
            return y, y_lens
        y = y[:, :self.num_out(w.shape[1])]
        return y[0] if one else y


def speed_perturb(waves, factors, lens=None, filter="kaiser_best", accumulate=None, out_dtype=torch.float32):
    """Speed perturbation as Kaiser's recipes do it with sox: row b of `waves` [B, n] (device, int16 / float32) resampled at
    ratio 1 / factors[b] and played back at the old rate, so that 1.1 gives shorter, faster audio and 0.9 longer, slower.  One
    launch for the batch.  Returns (out [B, longest output], out_lens [B]); a factor of 1.0 still passes through the filter."""
    factors = np.atleast_1d(np.asarray(factors, dtype=np.float64))
    if not (np.isfinite(factors).all() and (factors > 0).all()):
        raise ValueError("speed_perturb: factors must be finite and positive")
    return resample_rows(waves, 1.0 / factors, lens, filter, accumulate, out_dtype)


def resample(x, sr_orig, sr_new, filter="kaiser_best", device="cuda:0", **kwargs) -> np.ndarray:
    """Drop-in for resampy.resample(x, sr_orig, sr_new) as the reference calls it (dataset.py:126): numpy in, numpy out, 1-D or
    2-D input resampled along the last axis, int16 or float32 samples -> float32.  Raises the package's ValueError when the
    output would be empty.  `kwargs` go to Resampler (accumulate, out_dtype)."""
    x = np.asarray(x)
    if x.ndim not in (1, 2) or x.dtype not in (np.int16, np.float32):
        raise TypeError(f"resample: 1-D or 2-D int16 / float32 samples, got {x.ndim}-D {x.dtype}")
    rs = Resampler(sr_orig, sr_new, filter=filter, device=device, **kwargs)
    if rs.num_out(x.shape[-1]) < 1:
        raise ValueError(f"Input signal length={x.shape[-1]} is too small to resample from {sr_orig}->{sr_new}")
    dev = require_device(device, "resampling")
    return rs(torch.from_numpy(np.ascontiguousarray(x)).to(dev)).cpu().numpy()


class _CallableModule(types.ModuleType):
    """`xvector_amd.resample` names both this module and the drop-in function: the module is callable as that function, so
    `xvector_amd.resample(x, sr, 16000)` and `xvector_amd.resample.Resampler` both work."""

    def __call__(self, x, sr_orig, sr_new, filter="kaiser_best", **kwargs):
        return resample(x, sr_orig, sr_new, filter=filter, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
