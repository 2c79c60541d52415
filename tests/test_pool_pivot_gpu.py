"""Pooled std of a channel that is off in a whole utterance is exactly 0 in bf16x3 too.

The large-batch kernel's pooling partials (csrc/tdnn_pp16.hip, pool_rows) are sums of r - K about a pivot K.  With K taken from
a neighbouring utterance's frame, a dead channel's terms are all -K != 0 and fp32 rounding of n equal terms left ~|K| sqrt(eps)
of std (1e-5 at the bench batch, where the fp32 kernel and the fp64 reference give 0).  The pivot is the segment's own first
frame: K = 0 for such a channel and its sums are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_bf16x3_dead_channels_have_zero_std(sd42, synth, gpu_model):
    import xvector_amd as xa
    m3 = xa.XVectorModel(precision="bf16x3")
    m3.load_state_dict(sd42)
    m3 = m3.to(DEV).eval()
    B, T = 256, 300
    h = torch.as_tensor(synth.make_mfcc(B, T, seed=1000 + B)).to(DEV)
    for i in range(4):
        h = gpu_model.time_context_layers[i](h)
    got = m3.pooled_last_layer(h)
    assert m3.last_dispatch()[4] == "pp", "the batch did not reach the large-batch kernel"
    exact = gpu_model.pooled_last_layer(h)
    # channels whose pre-activation stays below zero by a margin in every frame of the utterance (fp32 on the device)
    W = sd42["time_context_layers.4.linear.weight"].to(DEV)
    b = sd42["time_context_layers.4.linear.bias"].to(DEV)
    pre_max = torch.stack([(h[u] @ W.T + b).max(dim=0).values for u in range(B)])
    scale = (h[0] @ W.T + b).abs().mean()
    dead = pre_max < -1e-2 * scale
    assert dead.sum() > 1000
    std3, std32 = got[:, 1500:], exact[:, 1500:]
    assert (std32[dead] == 0).all()
    assert (std3[dead] == 0).all(), f"{int((std3[dead] != 0).sum())} dead channels with a nonzero bf16x3 std, max {std3[dead].max().item():.3e}"
