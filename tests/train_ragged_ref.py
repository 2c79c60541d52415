"""The ragged training step restated for the tests (include/xvec_train.h, "Ragged batches"): what the valid frames alone give,
written in torch with autograd on per-utterance SLICES, so the padding cannot take part by construction.  Per layer: every
utterance is cut to its length and gathered alone (train_ref.gather), the valid rows of all utterances are concatenated and go
through F.relu(F.linear(...)) and ONE F.batch_norm over the N rows, then split back; pooling runs per utterance over its valid
frames; the loss is F.cross_entropy.  Gradients come from torch.autograd.grad, never from formulas.  In the dtype of the inputs
(the tests pass float64).  An utterance whose length is outside [span + 1, T] contributes no rows.  A plain module like
train_ref.py; the test files import it."""
import torch
import torch.nn.functional as F

import train_ref
from train_ref import CONTEXTS, EPS, MOMENTUM


def span_of(context):
    return context[-1] - context[0]


def valid_rows(lengths, T, context):
    """Valid output rows per utterance: l - span for span + 1 <= l <= T, otherwise 0."""
    s = span_of(context)
    return [l - s if s + 1 <= l <= T else 0 for l in lengths]


def fp32_product_error(rows, W, b):
    """A bound on the fp32 rounding error of rows @ W.T + b, whatever the order of the K + 1 additions:
    (K + 2) 2^-24 (|rows| @ |W|.T + |b|) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return (rows.shape[1] + 2) * 2.0 ** -24 * (rows.abs() @ W.abs().T + b.abs())


def layer_rows(xs, W, b, context, gamma=None, beta=None, running=None, eps=EPS):
    """One layer on a list of per-utterance inputs xs[b] [l_b, Cin] (l_b = 0: no rows).  dict(rows [N, K] the gathered input,
    pre, z, y [N, Cout], counts, ys: y split back per utterance); `running` = (running_mean, running_var) moves in place."""
    s = span_of(context)
    gathered = [train_ref.gather(x[None], context)[0] for x in xs if x.shape[0] > s]
    counts = [x.shape[0] - s if x.shape[0] > s else 0 for x in xs]
    rows = torch.cat(gathered, 0)
    pre = F.linear(rows, W, b)
    z = F.relu(pre)
    out = {"rows": rows, "pre": pre, "z": z, "y": z, "counts": counts}
    if gamma is not None:
        rm, rv = running if running is not None else (None, None)
        out["mean"] = z.mean(0)
        out["var"] = z.var(0, unbiased=False)
        out["y"] = F.batch_norm(z, rm, rv, gamma, beta, True, MOMENTUM, eps)
    out["ys"] = list(torch.split(out["y"], counts, 0))
    return out


def cut(x, lengths, lo=1):
    """x [B, T, C] -> the list of x[b, :l_b]; a length outside [lo, T] gives an empty slice."""
    T = x.shape[1]
    return [x[b, :l] if lo <= l <= T else x[b, :0] for b, l in enumerate(lengths)]


def pad(parts, Tp):
    """The list of [v_b, C] -> [B, Tp, C] with zeros on the invalid rows (what the calls write there)."""
    return torch.stack([torch.cat((p, p.new_zeros(Tp - p.shape[0], p.shape[1])), 0) for p in parts])


def layer(case, lengths, context, eps=EPS):
    """Everything the two ragged layer calls write, for a case dict(x, W, b, dy[, gamma, beta]) as tests/test_train_gpu.py's
    make_case draws it: dict(pre (valid rows), err (the fp32 bound on pre), z, y (padded with zeros), mean, var, dx, dW, db
    [, dgamma, dbeta]).  x and dy beyond the lengths are never touched."""
    bn = "gamma" in case
    B, T, _ = case["x"].shape
    Tp = T - span_of(context)
    x = case["x"]
    names = ["x", "W", "b"] + (["gamma", "beta"] if bn else [])
    leaves = {k: (x if k == "x" else case[k]).clone().requires_grad_(True) for k in names}
    s = span_of(context)
    f = layer_rows(cut(leaves["x"], lengths, s + 1), leaves["W"], leaves["b"], context, leaves.get("gamma"), leaves.get("beta"), eps=eps)
    dy = torch.cat([case["dy"][b, :v] for b, v in enumerate(f["counts"])], 0)
    grads = torch.autograd.grad(f["y"], [leaves[k] for k in names], dy)
    out = dict(zip(("dx", "dW", "db", "dgamma", "dbeta"), grads))
    with torch.no_grad():
        out.update(pre=f["pre"], err=fp32_product_error(f["rows"], case["W"], case["b"]), counts=f["counts"],
                   z=pad(torch.split(f["z"], f["counts"], 0), Tp), y=pad(f["ys"], Tp))
        if bn:
            out.update(mean=f["mean"], var=f["var"])
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def pool(parts):
    """(mean, unbiased std) per utterance over its own frames; an utterance without frames pools to zeros."""
    rows = []
    for p in parts:
        if p.shape[0] < 2:
            rows.append(p.new_zeros(2 * p.shape[1]))
        else:
            rows.append(torch.cat((p.mean(0), p.std(0))))
    return torch.stack(rows)


def tail_logits(parts, W6, b6, W7, b7, Wo, bo):
    h = pool(parts)
    h = F.relu(F.linear(h, W6, b6))
    h = F.relu(F.linear(h, W7, b7))
    return F.linear(h, Wo, bo)


def tail(case, lengths):
    """Everything the two ragged tail calls write, for a case of train_tail_ref.make_case: pooled, logits, loss and the
    gradients dy5 (zeros past the lengths), dW6 .. dbo, by autograd."""
    names = ["y5", "W6", "b6", "W7", "b7", "Wo", "bo"]
    y5 = case["y5"]
    leaves = {k: (y5 if k == "y5" else case[k]).clone().requires_grad_(True) for k in names}
    parts = cut(leaves["y5"], lengths, 2)
    pooled = pool(parts)
    logits = tail_logits(parts, *[leaves[k] for k in names[1:]])
    loss = F.cross_entropy(logits, case["labels"])
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    out = dict(zip(("dy5", "dW6", "db6", "dW7", "db7", "dWo", "dbo"), grads))
    out.update(pooled=pooled.detach(), logits=logits.detach(), loss=loss.detach())
    return out


def logits(sd, x, lengths, batch_norm=True, update_buffers=True, pre_margin=None):
    """train_ref.logits over a ragged batch.  `pre_margin`, a list, receives per layer min over the valid elements of
    |pre| / (the fp32 bound on its error)."""
    parts = cut(x, lengths)
    for i, ctx in enumerate(CONTEXTS):
        p = f"time_context_layers.{i}."
        running = None
        if batch_norm:
            running = (sd[p + "norm.running_mean"], sd[p + "norm.running_var"])
            if not update_buffers:
                running = tuple(t.clone() for t in running)
        f = layer_rows(parts, sd[p + "linear.weight"], sd[p + "linear.bias"], ctx,
                       sd[p + "norm.weight"] if batch_norm else None, sd[p + "norm.bias"] if batch_norm else None, running)
        if batch_norm and update_buffers:
            sd[p + "norm.num_batches_tracked"] += 1
        if pre_margin is not None:
            with torch.no_grad():
                pre_margin.append(float((f["pre"].abs() / fp32_product_error(f["rows"], sd[p + "linear.weight"],
                                                                             sd[p + "linear.bias"])).min()))
        parts = f["ys"]
    return tail_logits(parts, *[sd[k] for k in ("segment_layer6.weight", "segment_layer6.bias", "segment_layer7.weight",
                                               "segment_layer7.bias", "output.weight", "output.bias")])


def training_step(sd, x, lengths, labels, pre_margin=None):
    """loss and {key: gradient} of one ragged step; the buffers of `sd` move as in training mode (over the N valid rows)."""
    keys = train_ref.param_keys(sd)
    loss = F.cross_entropy(logits(sd, x, lengths, pre_margin=pre_margin), labels)
    grads = torch.autograd.grad(loss, [sd[k] for k in keys])
    return loss.detach(), dict(zip(keys, grads))


def adam_losses(sd, x, lengths, labels, steps, lr):
    """The losses of `steps` steps of torch.optim.Adam(lr) on one fixed ragged batch; `sd` is updated in place."""
    keys = train_ref.param_keys(sd)
    opt = torch.optim.Adam([sd[k] for k in keys], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.cross_entropy(logits(sd, x, lengths), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
