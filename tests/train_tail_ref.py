"""The tail of the training step restated for the tests (reference main.py:72-75, 99-100, 148): the formulas of
include/xvec_train.h (xvec_train_tail_forward / _backward, xvec_adam_step) in torch on the CPU, in the dtype of the inputs
(the tests pass float64), with the two ReLU masks of the backward as ARGUMENTS; the same tail written with torch ops and
autograd; and the Adam formulas.  A plain module like train_ref.py; the test files import it."""
import math

import torch
import torch.nn.functional as F


def tail_forward(y5, W6, b6, W7, b7, Wo, bo, labels):
    """dict(pooled, pre6, a6, pre7, a7, logits, rowloss, loss): pooled = (mean, unbiased std) over the frames."""
    tp = y5.shape[1]
    mean = y5.mean(1)
    std = torch.sqrt(((y5 - mean[:, None, :]) ** 2).sum(1) / (tp - 1))
    pooled = torch.cat((mean, std), 1)
    pre6 = pooled @ W6.T + b6
    a6 = pre6.clamp_min(0)
    pre7 = a6 @ W7.T + b7
    a7 = pre7.clamp_min(0)
    logits = a7 @ Wo.T + bo
    mx = logits.max(1, keepdim=True).values
    lse = mx[:, 0] + torch.log(torch.exp(logits - mx).sum(1))
    rowloss = lse - logits.gather(1, labels[:, None])[:, 0]
    return {"pooled": pooled, "pre6": pre6, "a6": a6, "pre7": pre7, "a7": a7, "logits": logits, "rowloss": rowloss,
            "loss": rowloss.sum() / y5.shape[0]}


def tail_backward(dloss, y5, W6, W7, Wo, labels, pooled, a6, a7, logits, mask6, mask7):
    """dict(dW6, db6, dW7, db7, dWo, dbo, dpooled, dy5) by the formulas of include/xvec_train.h; `mask6` / `mask7` [B, H] bool
    are [a6 > 0] / [a7 > 0] as the caller wants them taken (the backward is discontinuous in them)."""
    B, tp, c = y5.shape
    onehot = F.one_hot(labels, logits.shape[1]).to(logits.dtype)
    dlogits = dloss * (torch.softmax(logits, 1) - onehot) / B
    zero = torch.zeros((), dtype=y5.dtype)
    dz7 = torch.where(mask7, dlogits @ Wo, zero)
    dz6 = torch.where(mask6, dz7 @ W7, zero)
    dpooled = dz6 @ W6
    mean, std = pooled[:, :c], pooled[:, c:]
    dmean, dstd = dpooled[:, :c], dpooled[:, c:]
    fac = torch.where(std > 0, dstd / ((tp - 1) * torch.where(std > 0, std, torch.ones_like(std))), zero)
    dy5 = dmean[:, None, :] / tp + fac[:, None, :] * (y5 - mean[:, None, :])
    return {"dWo": dlogits.T @ a7, "dbo": dlogits.sum(0), "dW7": dz7.T @ a6, "db7": dz7.sum(0), "dW6": dz6.T @ pooled,
            "db6": dz6.sum(0), "dpooled": dpooled, "dy5": dy5}


def tail_autograd(y5, W6, b6, W7, b7, Wo, bo, labels):
    """The reference's own op sequence: mean, std, cat, linear, relu, linear, relu, linear, cross_entropy."""
    h = torch.cat((torch.mean(y5, 1), torch.std(y5, 1)), 1)
    h = F.relu(F.linear(h, W6, b6))
    h = F.relu(F.linear(h, W7, b7))
    return F.cross_entropy(F.linear(h, Wo, bo), labels)


def adam_step(p, g, m, v, lr, b1, b2, eps, t):
    """(p', m', v', u) of torch.optim.Adam's defaults at step count t >= 1; u = m' / (sqrt(v') / sqrt(1 - b2^t) + eps) is the
    normalised update, p' = p - lr / (1 - b1^t) u."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = m / (torch.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return p - (lr / (1 - b1 ** t)) * u, m, v, u


def make_case(B, tp, c, h, k, seed):
    """fp32 inputs of one tail case from ONE CPU generator, drawn in the order weights and biases (uniform in +-1/sqrt(fan_in)),
    labels (uniform over the classes), y5 (randn).  The order matters to the tests of the backward: with it the reference has
    no pre-activation within 1e-4 mean|pre| of zero in the four small SHAPES at seeds 1..3 and a share of at most 1.2e-4 in
    the two large ones (tests/test_train_tail.py checks this on the CPU); the cap of 2e-4 on that share is less than one
    element of a small case."""
    gen = torch.Generator().manual_seed(seed)
    uni = lambda fan_in, *shape: (torch.rand(*shape, generator=gen) * 2 - 1) / math.sqrt(fan_in)
    case = {"W6": uni(2 * c, h, 2 * c), "b6": uni(2 * c, h), "W7": uni(h, h, h), "b7": uni(h, h), "Wo": uni(h, k, h), "bo": uni(h, k)}
    case["labels"] = torch.randint(0, k, (B,), generator=gen)
    case["y5"] = torch.randn(B, tp, c, generator=gen)
    return case


# (B, Tp, C, H, K): the smallest at which each mechanism of csrc/train_tail.hip can go wrong
SHAPES = [
    (1, 2, 8, 8, 2),                  # the minimum everywhere
    (3, 7, 65, 33, 5),                # nothing divides anything: the element-wise paths, partial MFMA tiles
    (4, 26, 1500, 32, 7),             # the g10 fixture's tail
    (2, 300, 96, 16, 3),              # Tp beyond 256 frames
    (130, 5, 64, 129, 1211),          # B and H one past a 128 tile; a softmax row longer than a block; K odd
    (256, 4, 1500, 512, 1211),        # the model's own widths: the split over 2C = 3000; 6 MB of y5
]
