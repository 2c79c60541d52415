"""Training on the MI355X: the reference's `trainer.fit(model)` step (main.py:97-101, 148) on this package's model.

The five frame-level layers -- 99.7 % of a step's arithmetic -- run forward AND backward in HIP (include/xvec_train.h,
csrc/tdnn_train.hip): `tdnn_layer_train` is a torch.autograd.Function over the two C-ABI calls.  Statistics pooling, the three
segment-level Linear layers, the loss and Adam ride on torch ops on the same stream by default; with `tail="hip"` they run
in HIP too (csrc/train_tail.hip): pooling through loss as ONE autograd.Function over xvec_train_tail_forward / _backward, the
optimizer as `DeviceAdam` over xvec_adam_step.  Everything is fp32, the reference's own arithmetic.
There is no fallback: a CPU tensor or a reduced precision raise.

Dropout (`dropout_p` of the model, the reference's Linear -> ReLU -> Dropout -> BatchNorm): the forward product's epilogue
draws the mask from a counter-based generator (csrc/dropout_mask.h: Philox4x32-10 on (seed, stream, row, channel)), so no
mask is stored and a step is reproducible bit for bit.  It needs a seed: `XVectorTrainer(model, dropout_seed=...)`; layer i
of training step k uses stream 8 k + i.

Ragged batches: every entry point takes `lengths=` (valid frames per utterance of the padded batch x[B, T, C], as the
extraction calls do) and then goes through the length-masked calls (xvec_*_ragged): the step computes what the valid frames
alone would give, whatever the padding holds.  The layout stays padded, so the padding's arithmetic is still done.

    trainer = XVectorTrainer(model)                 # an XVectorModel on a HIP device; tail="hip": the whole step in HIP
    for batch in loader:                            # the reference's (samples, labels, ids)
        loss = trainer.step(batch)
    trainer.save_checkpoint("last.ckpt")            # XVectorModel.load_from_checkpoint reads it back
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import hip as _hip
from ._device import ptr, sized_workspace as _sized_workspace
from ._device import checker as _checker
from ._device import stream as _stream_ptr
from .model import TOTAL_CONTEXT, TdnnLayer, XVectorModel, _require_gpu

_check = _checker(_hip.lib.xvec_train_last_error)
_workspaces = {}        # (device index, stream) -> uint8 tensor; calls on one stream run in order and may share it


class _Lengths:
    """The valid input frames of one ragged call: `host` (a list of ints) and `dev` (the same as int32 on the device)."""

    def __init__(self, host, dev):
        self.host, self.dev = host, dev


def _host_lengths(lengths, B, lo, hi, what):
    """`lengths` (a list or a tensor) as a list of B ints in [lo, hi]; ValueError otherwise, before anything is launched."""
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().tolist()
    try:
        host = [int(v) for v in lengths]
    except TypeError:
        raise ValueError(f"{what}: lengths must be a list or a tensor of {B} integers") from None
    if len(host) != B or any(v != w for v, w in zip(host, lengths)):
        raise ValueError(f"{what}: lengths must be {B} integers, one per utterance; got {list(lengths)!r}")
    if min(host) < lo or max(host) > hi:
        raise ValueError(f"{what}: lengths must lie in [{lo}, T={hi}]; got {min(host)} .. {max(host)}")
    return host


def _stream_workspace(device, need):
    """The workspace of (device, current stream), grown to the `need` bytes a size query of xvec_train.h answered."""
    key = (device.index, _stream_ptr(device))
    refusal = lambda: _hip.XvecError(_hip.ERR_ARG, _hip.lib.xvec_train_last_error().decode())
    ws = _workspaces[key] = _sized_workspace(need, refusal, device, _workspaces.get(key))
    return ws


def _workspace(device, B, T, cin, cout, ctx, n_ctx):
    return _stream_workspace(device, _hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, ctx, n_ctx))


class _TdnnTrain(torch.autograd.Function):
    """y, batch_mean, batch_var = f(x, W, bias, gamma, beta): xvec_tdnn_train_forward / _backward.  Saved for the backward:
    x, z (the ReLU output), W, gamma and the batch statistics; y is not needed.  `dropout` = (p, seed, stream): the
    *_dropout calls, z is then the post-dropout value and the backward needs p alone."""

    @staticmethod
    def forward(ctx, x, W, bias, gamma, beta, context, eps, lengths_dev=None, dropout=None):
        B, T, cin = x.shape
        cout = W.shape[0]
        n_ctx = len(context)
        carr = (C.c_int32 * n_ctx)(*context)
        dev = x.device
        tp = T - (context[-1] - context[0])
        z = torch.empty((B, max(tp, 0), cout), dtype=torch.float32, device=dev)
        bn = gamma is not None
        y = torch.empty_like(z) if bn else z
        mean = torch.empty(cout if bn else 0, dtype=torch.float32, device=dev)
        var = torch.empty_like(mean)
        W, bias = W.detach().contiguous(), bias.detach().contiguous()
        if bn:
            gamma, beta = gamma.detach().contiguous(), beta.detach().contiguous()
        with torch.cuda.device(dev):
            ws = _workspace(dev, B, T, cin, cout, carr, n_ctx)
            args = (x.data_ptr(), B, T, cin, W.data_ptr(), bias.data_ptr(), cout, carr, n_ctx,
                    gamma.data_ptr() if bn else None, beta.data_ptr() if bn else None, eps, z.data_ptr(),
                    mean.data_ptr() if bn else None, var.data_ptr() if bn else None, y.data_ptr() if bn else None,
                    ws.data_ptr(), ws.numel(), _stream_ptr(dev))
            if dropout is not None:
                _check(_hip.lib.xvec_tdnn_train_forward_dropout(*args, None if lengths_dev is None else lengths_dev.data_ptr(),
                                                                *dropout))
            elif lengths_dev is None:
                _check(_hip.lib.xvec_tdnn_train_forward(*args))
            else:
                _check(_hip.lib.xvec_tdnn_train_forward_ragged(*args, lengths_dev.data_ptr()))
        ctx.save_for_backward(x, z, W, *((gamma, mean, var) if bn else ()))
        ctx.context, ctx.eps, ctx.bn, ctx.lengths_dev = tuple(context), eps, bn, lengths_dev
        ctx.dropout_p = None if dropout is None else dropout[0]
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, z, W = ctx.saved_tensors[:3]
        gamma, mean, var = ctx.saved_tensors[3:] if ctx.bn else (None, None, None)
        B, T, cin = x.shape
        cout = W.shape[0]
        n_ctx = len(ctx.context)
        carr = (C.c_int32 * n_ctx)(*ctx.context)
        dev = x.device
        dy = dy.contiguous().float()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W)
        db = torch.empty(cout, dtype=torch.float32, device=dev)
        dgamma = torch.empty_like(db) if ctx.bn else None
        dbeta = torch.empty_like(db) if ctx.bn else None
        with torch.cuda.device(dev):
            ws = _workspace(dev, B, T, cin, cout, carr, n_ctx)
            args = (dy.data_ptr(), x.data_ptr(), z.data_ptr(), B, T, cin, W.data_ptr(), cout, carr, n_ctx, ptr(gamma),
                    ptr(mean), ptr(var), ctx.eps, ptr(dx), dW.data_ptr(), db.data_ptr(), ptr(dgamma), ptr(dbeta),
                    ws.data_ptr(), ws.numel(), _stream_ptr(dev))
            if ctx.dropout_p is not None:
                _check(_hip.lib.xvec_tdnn_train_backward_dropout(
                    *args, None if ctx.lengths_dev is None else ctx.lengths_dev.data_ptr(), ctx.dropout_p))
            elif ctx.lengths_dev is None:
                _check(_hip.lib.xvec_tdnn_train_backward(*args))
            else:
                _check(_hip.lib.xvec_tdnn_train_backward_ragged(*args, ctx.lengths_dev.data_ptr()))
        return dx, dW, db, dgamma, dbeta, None, None, None, None


def _tail_workspace(device, B, tp, c, h, k):
    return _stream_workspace(device, _hip.lib.xvec_train_tail_workspace_bytes(B, tp, c, h, k))


class _TailTrain(torch.autograd.Function):
    """loss, logits = f(h5, W6, b6, W7, b7, Wo, bo, labels): xvec_train_tail_forward / _backward.  Saved for the backward:
    h5, the three weights, labels, and the call's own pooled, a6, a7 and logits.  logits is not differentiable (the loss is
    the only way into the graph); the incoming gradient of the loss stays on the device."""

    @staticmethod
    def forward(ctx, h5, W6, b6, W7, b7, Wo, bo, labels, lengths_dev=None):
        B, tp, c = h5.shape
        h, k = W6.shape[0], Wo.shape[0]
        dev = h5.device
        W6, b6, W7, b7, Wo, bo = (t.detach().contiguous() for t in (W6, b6, W7, b7, Wo, bo))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        pooled, a6, a7, logits, loss = new(B, 2 * c), new(B, h), new(B, h), new(B, k), new()
        with torch.cuda.device(dev):
            ws = _tail_workspace(dev, B, tp, c, h, k)
            args = (h5.data_ptr(), B, tp, c, W6.data_ptr(), b6.data_ptr(), h, W7.data_ptr(), b7.data_ptr(), Wo.data_ptr(),
                    bo.data_ptr(), k, labels.data_ptr(), pooled.data_ptr(), a6.data_ptr(), a7.data_ptr(), logits.data_ptr(),
                    loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
            if lengths_dev is None:
                _check(_hip.lib.xvec_train_tail_forward(*args))
            else:
                _check(_hip.lib.xvec_train_tail_forward_ragged(*args, lengths_dev.data_ptr()))
        ctx.save_for_backward(h5, W6, W7, Wo, labels, pooled, a6, a7, logits)
        ctx.lengths_dev = lengths_dev
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        h5, W6, W7, Wo, labels, pooled, a6, a7, logits = ctx.saved_tensors
        B, tp, c = h5.shape
        h, k = W6.shape[0], Wo.shape[0]
        dev = h5.device
        dloss = dloss.to(device=dev, dtype=torch.float32).contiguous()
        dy5 = torch.empty_like(h5) if ctx.needs_input_grad[0] else None
        dW6, dW7, dWo = torch.empty_like(W6), torch.empty_like(W7), torch.empty_like(Wo)
        db6, db7 = (torch.empty(h, dtype=torch.float32, device=dev) for _ in range(2))
        dbo = torch.empty(k, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _tail_workspace(dev, B, tp, c, h, k)
            args = (dloss.data_ptr(), h5.data_ptr(), B, tp, c, W6.data_ptr(), h, W7.data_ptr(), Wo.data_ptr(), k, labels.data_ptr(),
                    pooled.data_ptr(), a6.data_ptr(), a7.data_ptr(), logits.data_ptr(), None if dy5 is None else dy5.data_ptr(),
                    dW6.data_ptr(), db6.data_ptr(), dW7.data_ptr(), db7.data_ptr(), dWo.data_ptr(), dbo.data_ptr(), ws.data_ptr(),
                    ws.numel(), _stream_ptr(dev))
            if ctx.lengths_dev is None:
                _check(_hip.lib.xvec_train_tail_backward(*args))
            else:
                _check(_hip.lib.xvec_train_tail_backward_ragged(*args, ctx.lengths_dev.data_ptr()))
        return dy5, dW6, db6, dW7, db7, dWo, dbo, None, None


class DeviceAdam:
    """torch.optim.Adam with its defaults (amsgrad=False, weight_decay=0, not maximize) as ONE xvec_adam_step call per step
    (one launch per 32 tensors).  `state_dict()` / `load_state_dict()` use torch.optim.Adam's own layout -- state[i] = {step,
    exp_avg, exp_avg_sq} plus param_groups -- so a run can switch optimizer either way.  Parameters whose .grad is None are
    skipped, as torch skips them.  No fallback: `step()` raises on a parameter that is not fp32, not on a HIP device or not
    contiguous (checked where the pointers are taken: parameters may move between construction and the first step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        if not self.params:
            raise ValueError("DeviceAdam: no parameters")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or lr < 0.0 or eps < 0.0:
            raise ValueError(f"DeviceAdam: lr = {lr}, betas = {betas}, eps = {eps}")
        # the group's keys and defaults are torch.optim.Adam's own, whatever this torch's Adam carries (it holds no state
        # before its first step: this one only lends its parameter group, so that state_dict() loads into a real one)
        group = dict(torch.optim.Adam(self.params, lr=lr, betas=tuple(betas), eps=eps).param_groups[0])
        group["params"] = self.params
        self.param_groups = [group]
        self.state = {}                 # parameter index -> {"step": int, "exp_avg", "exp_avg_sq"}, from its first step on

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_().zero_()

    def _refuse_what_the_kernel_cannot_update(self):
        for i, p in enumerate(self.params):
            if p.dtype != torch.float32:
                raise RuntimeError(f"DeviceAdam: parameter {i} is {p.dtype}; the update runs in fp32 only")
            if p.device.type != "cuda":
                raise RuntimeError(f"DeviceAdam: parameter {i} is on {p.device}; it runs on a HIP device only (no CPU path)")
            if not p.is_contiguous():
                raise RuntimeError(f"DeviceAdam: parameter {i} is not contiguous")

    @torch.no_grad()
    def step(self):
        self._refuse_what_the_kernel_cannot_update()
        g = self.param_groups[0]
        calls = {}                      # (device index, t) -> parameter indices
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            if p.grad.dtype != torch.float32 or p.grad.device != p.device:
                raise RuntimeError(f"DeviceAdam: the gradient of parameter {i} is {p.grad.dtype} on {p.grad.device}")
            st = self.state.get(i)
            if st is None:
                st = self.state[i] = {"step": 0, "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                      "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
            calls.setdefault((p.device.index, st["step"] + 1), []).append(i)
        for (index, t), idx in calls.items():
            dev = torch.device("cuda", index)
            grads = [self.params[i].grad.contiguous() for i in idx]
            table = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
            lengths = (C.c_int64 * len(idx))(*[self.params[i].numel() for i in idx])
            with torch.cuda.device(dev):
                _check(_hip.lib.xvec_adam_step(
                    table([self.params[i] for i in idx]), table(grads), table([self.state[i]["exp_avg"] for i in idx]),
                    table([self.state[i]["exp_avg_sq"] for i in idx]), lengths, len(idx), float(g["lr"]), float(g["betas"][0]),
                    float(g["betas"][1]), float(g["eps"]), int(t), _stream_ptr(dev)))
            for i in idx:                  # counted once the update has been launched: a refused call leaves the state as it was
                self.state[i]["step"] = t

    def state_dict(self):
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.params)))
        state = {i: {"step": torch.tensor(float(st["step"])), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
                 for i, st in sorted(self.state.items())}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("DeviceAdam.load_state_dict: one parameter group over the same parameters is expected")
        g = groups[0]
        if g.get("amsgrad") or g.get("weight_decay") or g.get("maximize"):
            raise RuntimeError("DeviceAdam.load_state_dict: amsgrad, weight_decay and maximize are outside this build's scope")
        self.param_groups[0].update({k: v for k, v in g.items() if k != "params"})
        order = {pid: i for i, pid in enumerate(g["params"])}
        self.state = {}
        for pid, st in sd["state"].items():
            i = order[pid]
            p = self.params[i]
            moment = lambda t: t.detach().to(device=p.device, dtype=torch.float32).contiguous().clone().view_as(p)
            self.state[i] = {"step": int(st["step"]), "exp_avg": moment(st["exp_avg"]), "exp_avg_sq": moment(st["exp_avg_sq"])}


def tdnn_layer_train(x: torch.Tensor, layer: TdnnLayer, lengths=None, dropout=None) -> torch.Tensor:
    """`layer(x)` as the reference computes it under model.train() (tdnn_layer.py:26-41): x[B, T, in] ->
    y[B, T - span, out] with a graph through the layer's own parameters, BatchNorm on the batch statistics, and the
    layer's running_mean / running_var / num_batches_tracked updated as nn.BatchNorm1d updates them in training mode.

    `lengths` (a list or a tensor of B integers in [span + 1, T]): the valid frames of a padded batch.  Utterance b then has
    lengths[b] - span valid output frames -- the next layer's lengths -- which alone form the BatchNorm batch and receive
    gradients; the other rows of y are exactly 0, and nothing depends on what x holds past its lengths.

    `dropout` = (seed, stream), two integers below 2^64: a layer with dropout_p != 0 needs them.  They name the mask (include/
    xvec_train.h, "Dropout"): the same pair gives the same mask, whatever the batch; BatchNorm and the running statistics see
    the post-dropout activations, as torch's do.  A layer with dropout_p == 0 ignores them."""
    _require_gpu(x, "tdnn_layer_train")
    if layer.dropout_p and dropout is None:
        raise RuntimeError(f"tdnn_layer_train: dropout_p = {layer.dropout_p} needs dropout=(seed, stream): the mask is a "
                           f"function of them, there is no hidden generator state")
    if layer.dropout_p:
        seed, stream = (int(v) for v in dropout)
        if not (0 <= seed < 1 << 64 and 0 <= stream < 1 << 64):
            raise ValueError(f"tdnn_layer_train: dropout = {dropout!r}; seed and stream are integers in [0, 2^64)")
        dropout = (float(layer.dropout_p), seed, stream)
    else:
        dropout = None
    if x.dim() != 3 or x.shape[2] != layer.input_size:
        raise ValueError(f"tdnn_layer_train: expected x[B, T, {layer.input_size}], got {tuple(x.shape)}")
    W = layer.linear.weight
    if W.device != x.device or W.dtype != torch.float32:
        raise RuntimeError(f"tdnn_layer_train: parameters on {W.device}/{W.dtype}, input on {x.device}; move the model first")
    context = [int(c) for c in layer.context]
    x = x.float().contiguous()
    norm = layer.norm if layer.batch_norm else None
    span = context[-1] - context[0]
    n_rows = x.shape[0] * (x.shape[1] - span)
    if lengths is not None:
        if not isinstance(lengths, _Lengths):
            host = _host_lengths(lengths, x.shape[0], span + 1, x.shape[1], "tdnn_layer_train")
            lengths = _Lengths(host, torch.tensor(host, dtype=torch.int32).to(x.device))
        n_rows = sum(lengths.host) - x.shape[0] * span
    if norm is not None and n_rows == 1:
        raise ValueError("tdnn_layer_train: BatchNorm in training mode needs more than one row per channel")
    args = (x, W, layer.linear.bias, norm.weight if norm is not None else None, norm.bias if norm is not None else None, context,
            norm.eps if norm is not None else 0.0)
    if dropout is not None:
        y, mean, var = _TdnnTrain.apply(*args, None if lengths is None else lengths.dev, dropout)
    else:
        y, mean, var = _TdnnTrain.apply(*args) if lengths is None else _TdnnTrain.apply(*args, lengths.dev)
    if norm is not None and norm.track_running_stats:
        with torch.no_grad():
            norm.num_batches_tracked += 1
            m = norm.momentum if norm.momentum is not None else 1.0 / float(norm.num_batches_tracked)
            norm.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
            norm.running_var.mul_(1.0 - m).add_(var, alpha=m * n_rows / (n_rows - 1.0))
    return y


class XVectorTrainer:
    """The training half of the reference's LightningModule (main.py:97-131, 148) over an XVectorModel's own parameters.
    It does not look at `model.training`: `training_step` always uses batch statistics, `validation_step` always the
    running ones.

    `dropout_seed` (an integer in [0, 2^64)): required by a model with dropout_p != 0, ignored by one without.  Layer i of
    the k-th `training_step` call (k from 0) drops by the mask of (dropout_seed, stream 8 k + i); `dropout_state()` /
    `load_dropout_state()` carry (seed, k) across a checkpoint, so that a resumed run continues the sequence."""

    _HPARAMS = ("x_vec_extract_layer", "batch_size", "learning_rate", "augmentations_per_sample", "data_folder_path")

    def __init__(self, model: XVectorModel, tail: str = "torch", dropout_seed=None):
        if tail not in ("torch", "hip"):
            raise ValueError(f"XVectorTrainer: tail = {tail!r}; 'torch' (pooling, segment layers, loss and Adam on torch ops) "
                             f"or 'hip' (csrc/train_tail.hip)")
        if model.hparams["dropout_p"] and dropout_seed is None:
            raise RuntimeError(f"XVectorTrainer: dropout_p = {model.hparams['dropout_p']} needs a seed: pass dropout_seed= "
                               f"(the masks are a function of it and of the step count, which makes a run reproducible)")
        if dropout_seed is not None and not 0 <= int(dropout_seed) < 1 << 64:
            raise ValueError(f"XVectorTrainer: dropout_seed = {dropout_seed!r}; an integer in [0, 2^64)")
        if model.precision not in ("fp32", "f32"):
            raise RuntimeError(f"XVectorTrainer: precision {model.precision!r}; training runs in fp32 only")
        self.model = model
        self.tail = tail
        self.optimizer = None
        self._dropout_seed = int(dropout_seed) if model.hparams["dropout_p"] else None      # None: no dropout in this run
        self._dropout_step = 0              # training_step calls so far

    # ------------------------------------------------------------------ main.py:66-75 with a graph
    def _frames(self, x: torch.Tensor, lengths=None):
        """The five frame-level layers: x[B, T, in] -> h5[B, T - 14, 1500]; with `lengths`, (h5, the pooled lengths): every
        layer's lengths are the ones before less its span, uploaded as one table per step.  With dropout, layer i uses the
        stream 8 k + i of the step count k as it stands."""
        host = None
        if lengths is not None and x.dim() == 3:     # refused on the host first: a bad length never reaches a launch
            host = _host_lengths(lengths, x.shape[0], TOTAL_CONTEXT + 2, x.shape[1], "XVectorTrainer")
        _require_gpu(x, "XVectorTrainer")
        if x.dim() != 3 or x.shape[2] != self.model.hparams["input_size"]:
            raise ValueError(f"expected x[B, T, {self.model.hparams['input_size']}], got {tuple(x.shape)}")
        if x.shape[1] < TOTAL_CONTEXT + 2:
            raise ValueError(f"T={x.shape[1]}: training needs T >= {TOTAL_CONTEXT + 2} (two pooled frames for torch.std)")
        m = self.model
        h = x.float()
        drop = lambda i: None if self._dropout_seed is None else (self._dropout_seed, 8 * self._dropout_step + i)
        if lengths is None:
            for i, layer in enumerate(m.time_context_layers):
                h = tdnn_layer_train(h, layer, dropout=drop(i))
            return h
        table = [host]
        for layer in m.time_context_layers:
            span = int(layer.context[-1]) - int(layer.context[0])
            table.append([v - span for v in table[-1]])
        dev = torch.tensor(table, dtype=torch.int32).to(x.device)
        for i, layer in enumerate(m.time_context_layers):
            h = tdnn_layer_train(h, layer, _Lengths(table[i], dev[i]), drop(i))
        return h, _Lengths(table[-1], dev[-1])

    def logits(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        m = self.model
        # the tail, 0.3 % of the arithmetic, on torch ops (tail="hip": training_step goes through _TailTrain instead)
        if lengths is None:
            h = self._frames(x)
            h = torch.cat((torch.mean(h, 1), torch.std(h, 1)), 1)
        else:
            h, pooled_lengths = self._frames(x, lengths)
            h = self._masked_pool(h, pooled_lengths.dev)
        h = F.relu(F.linear(h, m.segment_layer6.weight, m.segment_layer6.bias))
        h = F.relu(F.linear(h, m.segment_layer7.weight, m.segment_layer7.bias))
        return F.linear(h, m.output.weight, m.output.bias)

    @staticmethod
    def _masked_pool(h, frames):
        """(mean, unbiased std) over the first frames[b] frames of h[b], by selection: what h holds past them does not matter.
        The std of a channel that is constant over them is 0 with a zero gradient, as torch.std's."""
        valid = (torch.arange(h.shape[1], device=h.device)[None, :] < frames[:, None])[:, :, None]
        n = frames.to(h.dtype)[:, None]
        zero = torch.zeros((), dtype=h.dtype, device=h.device)
        h = torch.where(valid, h, zero)                # selected BEFORE any arithmetic: the backward has no 0 * NaN either
        mean = h.sum(1) / n
        var = torch.where(valid, (h - mean[:, None, :]) ** 2, zero).sum(1) / (n - 1.0)
        std = torch.where(var > 0, torch.sqrt(torch.where(var > 0, var, torch.ones_like(var))), zero)
        return torch.cat((mean, std), 1)

    def training_step(self, batch, batch_index=0, lengths=None):
        try:
            return self._training_step(batch, lengths)
        finally:
            self._dropout_step += 1         # counted per call, whatever became of it: step k always means streams 8 k + i

    def _training_step(self, batch, lengths):
        samples, labels, ids = batch
        if self.tail == "hip":
            m = self.model
            tail = (m.segment_layer6.weight, m.segment_layer6.bias, m.segment_layer7.weight, m.segment_layer7.bias,
                    m.output.weight, m.output.bias)
            if lengths is None:
                h5 = self._frames(samples.float())
                loss, outputs = _TailTrain.apply(h5.contiguous(), *tail, labels.to(device=h5.device, dtype=torch.int64).contiguous())
            else:
                h5, pooled_lengths = self._frames(samples.float(), lengths)
                loss, outputs = _TailTrain.apply(h5.contiguous(), *tail, labels.to(device=h5.device, dtype=torch.int64).contiguous(),
                                                 pooled_lengths.dev)
            return {"loss": loss, "train_preds": outputs, "train_labels": labels, "train_id": ids}
        outputs = self.logits(samples.float(), lengths)
        loss = F.cross_entropy(outputs, labels.to(outputs.device))
        return {"loss": loss, "train_preds": outputs, "train_labels": labels, "train_id": ids}

    def validation_step(self, batch, batch_index=0, lengths=None):
        """main.py:120-124 as Lightning runs it (model.eval(), no graph): the HIP extraction path's logits, over the same
        `lengths` as the training step takes."""
        samples, labels, ids = batch
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                outputs = self.model(samples.float(), lengths)
                loss = F.cross_entropy(outputs, labels.to(outputs.device))
        finally:
            self.model.train(was_training)
        return {"loss": loss, "val_preds": outputs, "val_labels": labels, "val_id": ids}

    def configure_optimizers(self):
        if self.tail == "hip":
            return DeviceAdam(self.model.parameters(), lr=self.model.learning_rate)
        return torch.optim.Adam(self.model.parameters(), lr=self.model.learning_rate)

    def step(self, batch, lengths=None) -> torch.Tensor:
        """zero_grad, training_step, backward, optimizer step; returns the (detached) loss of the step."""
        if self.optimizer is None:
            self.optimizer = self.configure_optimizers()
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.training_step(batch, lengths=lengths)["loss"]
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def dropout_state(self):
        """{"seed", "step"} of a run with dropout -- what names the masks of the next training_step -- or None without."""
        return None if self._dropout_seed is None else {"seed": self._dropout_seed, "step": self._dropout_step}

    def load_dropout_state(self, state):
        """Continue the mask sequence of `dropout_state()` (a checkpoint's "xvec_dropout" entry)."""
        if self._dropout_seed is None:
            raise RuntimeError("XVectorTrainer.load_dropout_state: this run has no dropout (dropout_p == 0)")
        seed, step = int(state["seed"]), int(state["step"])
        if not 0 <= seed < 1 << 64 or step < 0:
            raise ValueError(f"XVectorTrainer.load_dropout_state: {state!r}")
        self._dropout_seed, self._dropout_step = seed, step

    def save_checkpoint(self, path):
        """A Lightning-shaped file: `state_dict` and `hyper_parameters` (what save_hyperparameters() stores, main.py:56).  A
        run with dropout adds "xvec_dropout", its `dropout_state()`; without dropout the file has the two keys alone."""
        m = self.model
        hp = dict(m.hparams)
        hp.update({k: getattr(m, k) for k in self._HPARAMS})
        ckpt = {"state_dict": {k: v.detach().cpu() for k, v in m.state_dict().items()}, "hyper_parameters": hp}
        if self._dropout_seed is not None:
            ckpt["xvec_dropout"] = self.dropout_state()
        torch.save(ckpt, path)
