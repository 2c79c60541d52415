"""Dropout in the training layers restated for the tests (include/xvec_train.h, "Dropout"): Philox4x32-10 and the keep rule in
numpy on uint64, written from the published round function and independent of csrc/dropout_mask.h; the layer with dropout
between ReLU and BatchNorm on top of train_ref.py, forward and backward by the header's formulas; and the same layer and the
whole step as torch ops with the mask INJECTED, for autograd.  In the dtype of the inputs (the tests pass float64).  A plain
module like train_ref.py; the test files import it."""
import numpy as np
import torch
import torch.nn.functional as F

import train_ref
from train_ref import CONTEXTS, EPS, MOMENTUM

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 values -> four uint32 arrays.  Ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key raised by (W0, W1) after
    each."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """An element is dropped iff its word < floor(p 2^32), p taken as the fp32 value the call receives."""
    return int(np.floor(float(np.float32(p)) * 2.0 ** 32))


def scale(p):
    """What a kept element is multiplied by: 1 / (1 - p) in double on the fp32 p, rounded to fp32."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def keep_mask(N, cout, p, seed, stream):
    """bool [N, cout]: element (n, c) is decided by word n & 3 of philox((c, n >> 2, stream_lo, stream_hi), (seed_lo, seed_hi))."""
    n = np.arange(N, dtype=np.uint64)[:, None]
    c = np.arange(cout, dtype=np.uint64)[None, :]
    words = philox4x32_10((c, n >> np.uint64(2), stream & MASK32, stream >> 32), (seed & MASK32, seed >> 32))
    word = np.choose((n & np.uint64(3)).astype(np.int64) + np.zeros_like(c, dtype=np.int64), words)
    return word.astype(np.uint64) >= np.uint64(threshold(p))


def layer_forward(x, W, b, context, keep, p, gamma=None, beta=None, eps=EPS):
    """train_ref.layer_forward with dropout after the ReLU: z = where(keep, relu(pre) * scale, 0); `keep` bool [B, T', Cout]."""
    pre = train_ref.gather(x, context) @ W.T + b
    z = torch.where(keep, pre.clamp_min(0) * scale(p), torch.zeros_like(pre))
    out = {"pre": pre, "z": z, "y": z}
    if gamma is not None:
        flat = z.reshape(-1, z.shape[-1])
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        invstd = 1.0 / torch.sqrt(var + eps)
        out.update(mean=mean, var=var, invstd=invstd, y=gamma * (z - mean) * invstd + beta)
    return out


def layer_backward(dy, x, z, mask, W, context, p, gamma=None, mean=None, var=None, eps=EPS):
    """train_ref.layer_backward on the post-dropout z and `mask` = [z > 0] as the caller wants it taken; dz -- and with it dW,
    db and dx -- times the scale.  dgamma and dbeta are as they are."""
    out = train_ref.layer_backward(dy, x, z, mask, W, context, gamma, mean, var, eps)
    for k in ("dz", "dW", "db", "dx"):
        out[k] = out[k] * scale(p)
    return out


def layer_autograd(x, W, b, context, keep, p, gamma=None, beta=None, eps=EPS):
    """The reference's op sequence with the mask injected: cat, linear, relu, * keep * scale, batch_norm."""
    h = F.relu(F.linear(train_ref.gather(x, context), W, b)) * keep.to(x.dtype) * scale(p)
    if gamma is not None:
        h = F.batch_norm(h.transpose(1, 2), None, None, gamma, beta, True, MOMENTUM, eps).transpose(1, 2)
    return h


def step_masks(B, T, widths, p, seed, step):
    """The five keep masks [B, T'_i, widths[i]] of training step `step`: layer i uses stream 8 step + i."""
    masks, t = [], T
    for i, ctx in enumerate(CONTEXTS):
        t -= ctx[-1] - ctx[0]
        masks.append(torch.from_numpy(keep_mask(B * t, widths[i], p, seed, 8 * step + i)).view(B, t, widths[i]))
    return masks


def logits(sd, x, p, seed, step):
    """train_ref.logits (batch statistics, the buffers of `sd` move) with the masks of (seed, step) injected."""
    widths = [sd[f"time_context_layers.{i}.linear.weight"].shape[0] for i in range(5)]
    masks = step_masks(x.shape[0], x.shape[1], widths, p, seed, step)
    h = x
    for i, ctx in enumerate(CONTEXTS):
        pre = f"time_context_layers.{i}."
        h = F.relu(F.linear(train_ref.gather(h, ctx), sd[pre + "linear.weight"], sd[pre + "linear.bias"]))
        h = h * masks[i].to(h.dtype) * scale(p)
        h = F.batch_norm(h.transpose(1, 2), sd[pre + "norm.running_mean"], sd[pre + "norm.running_var"], sd[pre + "norm.weight"],
                         sd[pre + "norm.bias"], True, MOMENTUM, EPS).transpose(1, 2)
        sd[pre + "norm.num_batches_tracked"] += 1
    h = torch.cat((torch.mean(h, 1), torch.std(h, 1)), 1)
    h = F.relu(F.linear(h, sd["segment_layer6.weight"], sd["segment_layer6.bias"]))
    h = F.relu(F.linear(h, sd["segment_layer7.weight"], sd["segment_layer7.bias"]))
    return F.linear(h, sd["output.weight"], sd["output.bias"])


def training_step(sd, x, labels, p, seed, step):
    """loss and {key: gradient} of one step with dropout; the buffers of `sd` move as in training mode."""
    keys = train_ref.param_keys(sd)
    loss = F.cross_entropy(logits(sd, x, p, seed, step), labels)
    grads = torch.autograd.grad(loss, [sd[k] for k in keys])
    return loss.detach(), dict(zip(keys, grads))
