"""Host plumbing shared by every module that calls the library (model, frontend, scoring, plda, evaluate, snorm, identify,
diarize, vbx, der, lda, augment, resample, vad, visualize, calibrate, fuse, bootstrap, report, train): error checks, the raw stream pointer, the pointer of an optional
tensor, the device-only guard, host data onto the device, the check of a device score matrix, the check of a host rec_start,
the pointer of a host int64 array, byte workspaces."""
from __future__ import annotations

import ctypes

import numpy as np
import torch


def checker(last_error_fn):
    """check(rc) raising XvecError with the text of ONE error channel (the library keeps one per module:
    xvec_last_error, xvec_mfcc_last_error, xvec_score_last_error, ...)."""
    from . import hip          # here, not at the top: hip binds a checker of its own while it loads

    def check(rc: int):
        if rc != hip.OK:
            raise hip.XvecError(rc, last_error_fn().decode())
    return check


def stream(device) -> int:
    """The raw hipStream_t of torch's current stream on `device`."""
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    """The device pointer of `t`; None (a null pointer) for an argument that was left out."""
    return None if t is None else t.data_ptr()


def require_device(device, what) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what} runs on a HIP device only (no CPU path)")
    return device


def dev_f64(a, device, keep_f32=False) -> torch.Tensor:
    """Array or tensor -> contiguous float64 tensor on `device`; with keep_f32 a float32 input stays float32."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        dtype = torch.float32 if keep_f32 and t.dtype == torch.float32 else torch.float64
        return t.to(device=device, dtype=dtype).contiguous()
    a = np.asarray(a)
    dtype = np.float32 if keep_f32 and a.dtype == np.float32 else np.float64
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device).contiguous()


def score_matrix(scores, what, shape="[n_rows, n_cols]", square=False) -> torch.Tensor:
    """`scores` as the library reads a score matrix: a float64 device tensor `shape`, not empty (`square`: and square), with
    unit column stride (copied only where it has another)."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise RuntimeError(f"{what} runs on a HIP device only (no CPU path): the scores must be a device tensor")
    if scores.dim() != 2 or scores.dtype != torch.float64:
        raise ValueError(f"{what}: expected a float64 {shape} score matrix")
    if square and (scores.shape[0] < 1 or scores.shape[0] != scores.shape[1]):
        raise ValueError(f"{what}: the score matrix must be square and not empty, got {tuple(scores.shape)}")
    if scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError(f"{what}: empty score matrix")
    return scores if scores.stride(1) == 1 and scores.stride(0) >= scores.shape[1] else scores.contiguous()


def rec_start(rec_start, n, what, rows, unit) -> np.ndarray:
    """`rec_start` as the library reads it on the host: contiguous int64 [n_rec + 1] rising from 0 to `n`, no recording empty.
    `rows` says what the n are, `unit` what a recording is made of."""
    rs = np.ascontiguousarray(np.asarray(rec_start), dtype=np.int64)
    if rs.ndim != 1 or rs.shape[0] < 2 or rs[0] != 0 or rs[-1] != n or (np.diff(rs) < 1).any():
        raise ValueError(f"{what}: rec_start must rise from 0 to the {n} {rows}, a {unit} or more per recording")
    return rs


def i64_ptr(a: np.ndarray):
    """The `const int64_t*` of a contiguous host int64 array (rec_start, class_start); `a` must outlive the call."""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def byte_workspace(need, device, cached=None) -> torch.Tensor:
    """`cached` if it holds `need` bytes, else a new uint8 tensor (never an empty one: its pointer would be null)."""
    if cached is not None and cached.numel() >= need:
        return cached
    return torch.empty(max(1, int(need)), dtype=torch.uint8, device=device)


def sized_workspace(need, refusal, device, cached=None) -> torch.Tensor:
    """byte_workspace for the `need` bytes a *_workspace_bytes query answered; 0 is the query's refusal of its arguments and
    raises the exception that `refusal()` returns."""
    if need == 0:
        raise refusal()
    return byte_workspace(int(need), device, cached)
