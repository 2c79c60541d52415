"""Host plumbing shared by the modules that call the library (model, frontend, scoring, plda, evaluate): error
checks, the raw stream pointer, the device-only guard, host data onto the device, byte workspaces."""
from __future__ import annotations

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


def byte_workspace(need, device, cached=None) -> torch.Tensor:
    """`cached` if it holds `need` bytes, else a new uint8 tensor (never an empty one: its pointer would be null)."""
    if cached is not None and cached.numel() >= need:
        return cached
    return torch.empty(max(1, int(need)), dtype=torch.uint8, device=device)
