#!/usr/bin/env python3
"""Generate g10_train.npz by running the REFERENCE's own training step (main.py:97-101, 148) in float64.

Runs only where the reference checkout is present (as make_golden.py, whose stand-ins for the third-party packages that are
not installed are reused).  The reference's `main.XVectorModel` at reduced width (hidden_size 64, x_vector_size 32,
num_classes 7; its 1500 and 3000 are fixed) gets this repo's synthetic weights by seed, is put in `.train()` and `.double()`,
and runs `training_step` on one batch B = 4, T = 40 -- in float64, so the fixture is the reference's arithmetic without its
rounding.  `training_step` casts its samples with `.float()`; the samples are float32 VALUES held in a float64 tensor whose
`.float()` hands them back as they are (the cast would be the identity on them).  Nothing of the reference is copied: the
fixture holds seeds, inputs and recorded results.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train.py

g10_train.npz
  seed_w, seed_x, seed_y, B, T, hidden_size, x_vector_size, num_classes, lr
  x float32 [B, T, 24], labels int64 [B]
  loss                          float64, training_step's loss
  grad/<parameter>              float64, the gradient after loss.backward(); for the two large matrices
                                (time_context_layers.4.linear.weight [1500, 64], segment_layer6.weight [32, 3000]) instead
  grad_rows/<parameter>         the rows listed in grad_rows_idx/<parameter>, plus
  grad_rowsum/, grad_colsum/    the whole tensor's sums over its columns and over its rows
  buf/<buffer>                  running_mean, running_var (float64) and num_batches_tracked after that one step
  adam_losses float64 [3]       the losses of three optimizer steps (configure_optimizers) on that batch from the same start
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SEED_W, SEED_X, SEED_Y = 31, 32, 33
B, T = 4, 40
KW = dict(input_size=24, hidden_size=64, num_classes=7, x_vector_size=32)
LARGE = {"time_context_layers.4.linear.weight": [0, 1, 2, 3, 700, 749, 750, 1498, 1499],
         "segment_layer6.weight": [0, 15, 31]}


class _AsIs(torch.Tensor):
    def float(self):
        return self.as_subclass(torch.Tensor)


def fresh_model(main, synth):
    m = main.XVectorModel(**KW)
    sd = mg.to_t(synth.make_state_dict(seed=SEED_W, **KW))
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if not k.startswith(("accuracy", "dataset"))], res
    return m.double().train()


def main_():
    assert os.path.isdir(mg.REF), "reference not present: fixtures can only be generated in the build container"
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    main = importlib.import_module("main")
    synth = mg.load_pkg().synth
    torch.set_num_threads(8)

    x32 = synth.make_mfcc(B, T, seed=SEED_X)
    labels = torch.from_numpy(np.random.default_rng(SEED_Y).integers(0, KW["num_classes"], B))
    batch = (torch.from_numpy(x32).double().as_subclass(_AsIs), labels, [f"id{i}" for i in range(B)])

    model = fresh_model(main, synth)
    out = model.training_step(batch, 0)
    assert out["loss"].dtype == torch.float64 and out["train_preds"].dtype == torch.float64
    out["loss"].backward()
    g = {"seed_w": SEED_W, "seed_x": SEED_X, "seed_y": SEED_Y, "B": B, "T": T, "lr": model.learning_rate,
         "x": x32, "labels": labels.numpy(), "loss": out["loss"].detach().numpy()}
    g.update(KW)
    for name, p in model.named_parameters():
        grad = p.grad.detach().numpy()
        if name in LARGE:
            idx = np.array(LARGE[name], dtype=np.int32)
            g["grad_rows_idx/" + name] = idx
            g["grad_rows/" + name] = grad[idx]
            g["grad_rowsum/" + name] = grad.sum(1)
            g["grad_colsum/" + name] = grad.sum(0)
        else:
            g["grad/" + name] = grad
    for name, b in model.named_buffers():
        g["buf/" + name] = b.detach().numpy()

    model = fresh_model(main, synth)
    opt = model.configure_optimizers()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model.training_step(batch, 0)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[0] == float(g["loss"])
    g["adam_losses"] = np.array(losses)
    mg.save("g10_train.npz", **g)


if __name__ == "__main__":
    main_()
