"""What the GPU tests of the frame-level (TDNN) layers share: handles created under a dispatch-knob setting, the fp64 oracle
of one layer, the worst-frame error and a layer's input chain.  A plain module like plda_em_ref.py; the test files import it."""
import os

import pytest
import torch

import xvector_oracle as oracle
from conftest import float_params

DEV = "cuda:0"
# every knob read_policy (csrc/xvec_api.hip) reads, once per handle in xvec_create (tests/test_support_modules.py ties the two)
KNOBS = ("XVEC_BLOCKS_PER_CU", "XVEC_PP", "XVEC_PP_MIN_TENTHS", "XVEC_PP_CU_PCT", "XVEC_WINOGRAD", "XVEC_SPLIT3",
         "XVEC_SPLIT3_MIN_ROWS", "XVEC_WINO_SPLIT3", "XVEC_WINO_SPLIT3_MIN_ROWS")


def make_model(sd, env=None, precision="fp32", **ctor_kwargs):
    """A model on DEV with the weights `sd` whose handle is created now, under the knobs `env` and no others: whatever the
    calling environment sets for a knob does not reach the handle, and the environment is as it was afterwards."""
    import xvector_amd as xa
    env = env or {}
    assert set(env) <= set(KNOBS), f"not a dispatch knob: {sorted(set(env) - set(KNOBS))}"
    m = xa.XVectorModel(precision=precision, **ctor_kwargs)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env)
        m._engine(torch.device(DEV))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return m


@pytest.fixture(scope="module")
def p64(sd42):
    return oracle.cast_params(float_params(sd42), torch.float64)


def oracle_layer(x_cpu, p64, layer, batch_norm=True, chunk=32):
    """fp64 oracle of one layer on fp32 input, a few utterances at a time (memory)."""
    outs = []
    for lo in range(0, x_cpu.shape[0], chunk):
        outs.append(oracle.tdnn_layer(x_cpu[lo:lo + chunk].double(), p64, f"time_context_layers.{layer}.",
                                      oracle.CONTEXTS[layer], batch_norm))
    return torch.cat(outs)


def worst_rel(got, ref64):
    """Worst norm-wise relative error of a frame (a row of the last dimension)."""
    g = got.double().cpu().reshape(-1, got.shape[-1])
    r = ref64.reshape(-1, ref64.shape[-1])
    return ((g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)).max().item()


def workspace_layout(m, total_frames, n_utts):
    """The library's workspace layout (xvec_workspace_layout) for a batch of `n_utts` utterances and `total_frames` frames."""
    import ctypes
    from xvector_amd import hip
    lay = hip.WsLayout()
    hip.check(hip.lib.xvec_workspace_layout(m._engine(torch.device(DEV)).h, total_frames, n_utts, ctypes.byref(lay)))
    return lay


def workspace_rows(m, xg, lengths, which):
    """The compact rows [sum(len - 14), hidden] that the whole path leaves in activation buffer "a" (layer 3's output) or "b"
    (layer 4's) of the workspace, with the padded channels cut off: layer l writes buffer l & 1 (csrc/xvec_api.hip, plan_stack),
    and the pooled mode runs no segment layer, which would reuse them.  (Layer 2's rows are overwritten by layer 4, and a wrong
    bit in them changes layer 3's.)  The workspace is filled with 0xFF bytes before m.pooled(xg, lengths=lengths) runs: a row
    that no layer wrote reads as NaN.  (What that fill shows is limited: layer 1 writes buffer "a" and layer 2 buffer "b" before
    layers 3 and 4 do, over more rows, so a row layer 3 or 4 skipped holds an earlier layer's finite values, and a NaN a layer
    READS comes out of its ReLU as 0, fmaxf(NaN, 0).  Both show against a reference of the rows, not in isfinite.)
    lengths None: a fixed-length batch.  which: "a", "b", or "ab" for both buffers of the one run."""
    B, T = xg.shape[0], xg.shape[1]
    lens = [T] * B if lengths is None else [int(n) for n in lengths]
    eng = m._engine(torch.device(DEV))
    eng.ensure_workspace(sum(lens), B)
    eng.workspace.fill_(0xFF)
    m.pooled(xg, lengths=lengths)
    torch.cuda.synchronize()
    lay = workspace_layout(m, sum(lens), B)
    n_rows, nh, hid = sum(n - 14 for n in lens), lay.hidden_n_pad, m.hparams["hidden_size"]
    rows = [eng.workspace[at: at + n_rows * nh * 4].view(torch.float32).reshape(-1, nh)[:, :hid].clone()
            for at in ({"a": lay.act_a, "b": lay.act_b}[w] for w in which)]
    return rows[0] if len(which) == 1 else tuple(rows)           # which = "ab": both buffers of the one run


def layer_input(m, synth, B, T, layer, seed):
    """fp32 input of `layer`: the chain of `m`'s layers before it, on the GPU."""
    h = torch.as_tensor(synth.make_mfcc(B, T, seed=seed)).to(DEV)
    for i in range(layer):
        h = m.time_context_layers[i](h)
    return h
