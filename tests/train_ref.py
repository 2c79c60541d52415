"""The training step restated for the tests (reference tdnn_layer.py:26-41, main.py:59-75, 97-101, 148): the formulas of
include/xvec_train.h in torch on the CPU, in the dtype of the inputs (the tests pass float64), with the ReLU mask of the
backward as an ARGUMENT, and the same layer and the whole step written with torch ops and autograd.  A plain module like
plda_em_ref.py; the test files import it."""
import torch
import torch.nn.functional as F

CONTEXTS = [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]]
EPS = 1e-5
MOMENTUM = 0.1


def gather(x, context):
    """x[B, T, C] -> x_ctx[B, T', taps * C], the reference's torch.cat(get_time_context(x, context), 2)."""
    span = context[-1] - context[0]
    tp = x.shape[1] - span
    return torch.cat([x[:, c - context[0]: c - context[0] + tp, :] for c in context], 2)


def layer_forward(x, W, b, context, gamma=None, beta=None, eps=EPS):
    """dict(pre, z, mean, var (biased), invstd, y) of one layer on batch statistics; without gamma y is z."""
    pre = gather(x, context) @ W.T + b
    z = pre.clamp_min(0)
    out = {"pre": pre, "z": z, "y": z}
    if gamma is not None:
        flat = z.reshape(-1, z.shape[-1])
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        invstd = 1.0 / torch.sqrt(var + eps)
        out.update(mean=mean, var=var, invstd=invstd, y=gamma * (z - mean) * invstd + beta)
    return out


def layer_backward(dy, x, z, mask, W, context, gamma=None, mean=None, var=None, eps=EPS):
    """dict(dx, dW, db, dgamma, dbeta, dz) by the formulas of include/xvec_train.h; `mask` [B, T', Cout] bool is [z > 0]
    as the caller wants it taken (the backward is discontinuous in it)."""
    B, T, cin = x.shape
    cout = W.shape[0]
    n = z.shape[0] * z.shape[1]
    out = {}
    if gamma is not None:
        invstd = 1.0 / torch.sqrt(var + eps)
        xhat = (z - mean) * invstd
        dbeta = dy.reshape(n, cout).sum(0)
        dgamma = (dy * xhat).reshape(n, cout).sum(0)
        dz = gamma * invstd * (dy - dbeta / n - xhat * dgamma / n)
        out.update(dbeta=dbeta, dgamma=dgamma)
    else:
        dz = dy.clone()
    dz = torch.where(mask, dz, torch.zeros_like(dz))
    out["dz"] = dz
    out["db"] = dz.reshape(n, cout).sum(0)
    out["dW"] = dz.reshape(n, cout).T @ gather(x, context).reshape(n, -1)
    dx = torch.zeros_like(x)
    tp = z.shape[1]
    for i, c in enumerate(context):
        off = c - context[0]
        dx[:, off: off + tp, :] += dz @ W[:, i * cin: (i + 1) * cin]
    out["dx"] = dx
    return out


def layer_autograd(x, W, b, context, gamma=None, beta=None, eps=EPS):
    """The reference's own op sequence for one layer in training mode: cat, linear, relu, batch_norm."""
    h = F.relu(F.linear(gather(x, context), W, b))
    if gamma is not None:
        h = F.batch_norm(h.transpose(1, 2), None, None, gamma, beta, True, MOMENTUM, eps).transpose(1, 2)
    return h


def logits(sd, x, batch_norm=True, update_buffers=True):
    """main.py:66-75 under model.train() on a state_dict (reference keys); updates the BatchNorm buffers of `sd` in place."""
    h = x
    for i, ctx in enumerate(CONTEXTS):
        pre = f"time_context_layers.{i}."
        h = F.relu(F.linear(gather(h, ctx), sd[pre + "linear.weight"], sd[pre + "linear.bias"]))
        if batch_norm:
            rm, rv = sd[pre + "norm.running_mean"], sd[pre + "norm.running_var"]
            if not update_buffers:
                rm, rv = rm.clone(), rv.clone()
            h = F.batch_norm(h.transpose(1, 2), rm, rv, sd[pre + "norm.weight"], sd[pre + "norm.bias"], True, MOMENTUM,
                             EPS).transpose(1, 2)
            if update_buffers:
                sd[pre + "norm.num_batches_tracked"] += 1
    h = torch.cat((torch.mean(h, 1), torch.std(h, 1)), 1)
    h = F.relu(F.linear(h, sd["segment_layer6.weight"], sd["segment_layer6.bias"]))
    h = F.relu(F.linear(h, sd["segment_layer7.weight"], sd["segment_layer7.bias"]))
    return F.linear(h, sd["output.weight"], sd["output.bias"])


PARAM_SUFFIXES = ("linear.weight", "linear.bias", "norm.weight", "norm.bias", "segment_layer6.weight", "segment_layer6.bias",
                  "segment_layer7.weight", "segment_layer7.bias", "output.weight", "output.bias")


def cast_state(sd, dtype):
    """A private copy of a state_dict (numpy or torch values): floating entries in `dtype`, parameters requiring grad."""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v).clone()
        if t.is_floating_point():
            t = t.to(dtype)
            if k.endswith(PARAM_SUFFIXES):
                t.requires_grad_(True)
        out[k] = t
    return out


def param_keys(sd):
    return [k for k, v in sd.items() if v.requires_grad]


def training_step(sd, x, labels):
    """loss and {key: gradient} of main.py:97-101 + loss.backward(); the buffers of `sd` move as in training mode."""
    keys = param_keys(sd)
    loss = F.cross_entropy(logits(sd, x), labels)
    grads = torch.autograd.grad(loss, [sd[k] for k in keys])
    return loss.detach(), dict(zip(keys, grads))


def adam_losses(sd, x, labels, steps, lr):
    """The losses of `steps` steps of torch.optim.Adam(lr) on one fixed batch (main.py:148); `sd` is updated in place."""
    keys = param_keys(sd)
    opt = torch.optim.Adam([sd[k] for k in keys], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.cross_entropy(logits(sd, x), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
