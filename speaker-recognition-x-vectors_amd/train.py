"""Training on the MI355X: the reference's `trainer.fit(model)` step (main.py:97-101, 148) on this package's model.

The five frame-level layers -- 99.7 % of a step's arithmetic -- run forward AND backward in HIP (include/xvec_train.h,
csrc/tdnn_train.hip): `tdnn_layer_train` is a torch.autograd.Function over the two C-ABI calls.  Statistics pooling, the three
segment-level Linear layers, the loss and Adam ride on torch ops on the same stream for now (the next
row).  Everything is fp32, the reference's own arithmetic.  There is no fallback: a CPU tensor, dropout or a reduced
precision raise.

    trainer = XVectorTrainer(model)                 # an XVectorModel on a HIP device
    for batch in loader:                            # the reference's (samples, labels, ids)
        loss = trainer.step(batch)
    trainer.save_checkpoint("last.ckpt")            # XVectorModel.load_from_checkpoint reads it back
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import hip as _hip
from ._device import byte_workspace as _byte_workspace
from ._device import checker as _checker
from ._device import stream as _stream_ptr
from .model import TOTAL_CONTEXT, TdnnLayer, XVectorModel, _require_gpu

_check = _checker(_hip.lib.xvec_train_last_error)
_workspaces = {}        # (device index, stream) -> uint8 tensor; calls on one stream run in order and may share it


def _workspace(device, B, T, cin, cout, ctx, n_ctx):
    need = int(_hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, ctx, n_ctx))
    if need == 0:
        raise _hip.XvecError(_hip.ERR_ARG, _hip.lib.xvec_train_last_error().decode())
    key = (device.index, _stream_ptr(device))
    ws = _workspaces[key] = _byte_workspace(need, device, _workspaces.get(key))
    return ws


class _TdnnTrain(torch.autograd.Function):
    """y, batch_mean, batch_var = f(x, W, bias, gamma, beta): xvec_tdnn_train_forward / _backward.  Saved for the backward:
    x, z (the ReLU output), W, gamma and the batch statistics; y is not needed."""

    @staticmethod
    def forward(ctx, x, W, bias, gamma, beta, context, eps):
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
            _check(_hip.lib.xvec_tdnn_train_forward(
                x.data_ptr(), B, T, cin, W.data_ptr(), bias.data_ptr(), cout, carr, n_ctx,
                gamma.data_ptr() if bn else None, beta.data_ptr() if bn else None, eps, z.data_ptr(),
                mean.data_ptr() if bn else None, var.data_ptr() if bn else None, y.data_ptr() if bn else None,
                ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
        ctx.save_for_backward(x, z, W, *((gamma, mean, var) if bn else ()))
        ctx.context, ctx.eps, ctx.bn = tuple(context), eps, bn
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
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            ws = _workspace(dev, B, T, cin, cout, carr, n_ctx)
            _check(_hip.lib.xvec_tdnn_train_backward(
                dy.data_ptr(), x.data_ptr(), z.data_ptr(), B, T, cin, W.data_ptr(), cout, carr, n_ctx, ptr(gamma),
                ptr(mean), ptr(var), ctx.eps, ptr(dx), dW.data_ptr(), db.data_ptr(), ptr(dgamma), ptr(dbeta),
                ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
        return dx, dW, db, dgamma, dbeta, None, None


def tdnn_layer_train(x: torch.Tensor, layer: TdnnLayer) -> torch.Tensor:
    """`layer(x)` as the reference computes it under model.train() (tdnn_layer.py:26-41): x[B, T, in] ->
    y[B, T - span, out] with a graph through the layer's own parameters, BatchNorm on the batch statistics, and the
    layer's running_mean / running_var / num_batches_tracked updated as nn.BatchNorm1d updates them in training mode."""
    _require_gpu(x, "tdnn_layer_train")
    if layer.dropout_p:
        raise RuntimeError(f"tdnn_layer_train: dropout_p = {layer.dropout_p} is outside this build's scope (only 0)")
    if x.dim() != 3 or x.shape[2] != layer.input_size:
        raise ValueError(f"tdnn_layer_train: expected x[B, T, {layer.input_size}], got {tuple(x.shape)}")
    W = layer.linear.weight
    if W.device != x.device or W.dtype != torch.float32:
        raise RuntimeError(f"tdnn_layer_train: parameters on {W.device}/{W.dtype}, input on {x.device}; move the model first")
    context = [int(c) for c in layer.context]
    x = x.float().contiguous()
    norm = layer.norm if layer.batch_norm else None
    n_rows = x.shape[0] * (x.shape[1] - (context[-1] - context[0]))
    if norm is not None and n_rows == 1:
        raise ValueError("tdnn_layer_train: BatchNorm in training mode needs more than one row per channel")
    y, mean, var = _TdnnTrain.apply(x, W, layer.linear.bias, norm.weight if norm is not None else None,
                                    norm.bias if norm is not None else None, context, norm.eps if norm is not None else 0.0)
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
    running ones."""

    _HPARAMS = ("x_vec_extract_layer", "batch_size", "learning_rate", "augmentations_per_sample", "data_folder_path")

    def __init__(self, model: XVectorModel):
        if model.hparams["dropout_p"]:
            raise RuntimeError(f"XVectorTrainer: dropout_p = {model.hparams['dropout_p']} is outside this build's scope (only 0)")
        if model.precision not in ("fp32", "f32"):
            raise RuntimeError(f"XVectorTrainer: precision {model.precision!r}; training runs in fp32 only")
        self.model = model
        self.optimizer = None

    # ------------------------------------------------------------------ main.py:66-75 with a graph
    def logits(self, x: torch.Tensor) -> torch.Tensor:
        _require_gpu(x, "XVectorTrainer")
        if x.dim() != 3 or x.shape[2] != self.model.hparams["input_size"]:
            raise ValueError(f"expected x[B, T, {self.model.hparams['input_size']}], got {tuple(x.shape)}")
        if x.shape[1] < TOTAL_CONTEXT + 2:
            raise ValueError(f"T={x.shape[1]}: training needs T >= {TOTAL_CONTEXT + 2} (two pooled frames for torch.std)")
        m = self.model
        h = x.float()
        for layer in m.time_context_layers:
            h = tdnn_layer_train(h, layer)
        # the tail, 0.3 % of the arithmetic, on torch ops (next row)
        h = torch.cat((torch.mean(h, 1), torch.std(h, 1)), 1)
        h = F.relu(F.linear(h, m.segment_layer6.weight, m.segment_layer6.bias))
        h = F.relu(F.linear(h, m.segment_layer7.weight, m.segment_layer7.bias))
        return F.linear(h, m.output.weight, m.output.bias)

    def training_step(self, batch, batch_index=0):
        samples, labels, ids = batch
        outputs = self.logits(samples.float())
        loss = F.cross_entropy(outputs, labels.to(outputs.device))
        return {"loss": loss, "train_preds": outputs, "train_labels": labels, "train_id": ids}

    def validation_step(self, batch, batch_index=0):
        """main.py:120-124 as Lightning runs it (model.eval(), no graph): the HIP extraction path's logits."""
        samples, labels, ids = batch
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                outputs = self.model(samples.float())
                loss = F.cross_entropy(outputs, labels.to(outputs.device))
        finally:
            self.model.train(was_training)
        return {"loss": loss, "val_preds": outputs, "val_labels": labels, "val_id": ids}

    def configure_optimizers(self):
        return torch.optim.Adam(self.model.parameters(), lr=self.model.learning_rate)

    def step(self, batch) -> torch.Tensor:
        """zero_grad, training_step, backward, optimizer step; returns the (detached) loss of the step."""
        if self.optimizer is None:
            self.optimizer = self.configure_optimizers()
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.training_step(batch)["loss"]
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def save_checkpoint(self, path):
        """A Lightning-shaped file: `state_dict` and `hyper_parameters` (what save_hyperparameters() stores, main.py:56)."""
        m = self.model
        hp = dict(m.hparams)
        hp.update({k: getattr(m, k) for k in self._HPARAMS})
        torch.save({"state_dict": {k: v.detach().cpu() for k, v in m.state_dict().items()}, "hyper_parameters": hp}, path)
