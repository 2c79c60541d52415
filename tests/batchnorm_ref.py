"""BatchNorm as a trained checkpoint has it, for the tests of the inference paths: a generator that calibrates a synthetic
state_dict on a batch (running statistics that are the real channel statistics, dead and rarely-on channels, gammas of either
sign, zero and denormal-small), the fp64 layer with a free eps, the folded fp32 constants as pack.hip computes them, and a CPU
restatement of plain bf16's deferred-BatchNorm arithmetic.  A plain module like tdnn_support.py; the test files import it.

The kernels fold eval BatchNorm (tdnn_layer.py:36-39) into y = relu(z + bias) * scale + shift, scale = gamma / sqrt(var + eps),
shift = beta - mean * scale.  synth.make_state_dict draws gamma in U(0.5, 1.5), var in U(0.5, 2): scale is positive and of order
one, eps is invisible and nothing cancels.  A checkpoint is different in each of these."""
import os

import numpy as np
import torch

import xvector_oracle as oracle

SCALE_GUARD = 1e-18            # pack.hip, pack_rows_kernel: |scale| below this reads as "the channel carries nothing"
TINY_GAMMAS = (1e-30, 1e-42)   # the second is denormal in fp32
DEAD_SHARE, RARE_SHARE, ZERO_SHARE, NEG_SHARE = 0.02, 0.04, 0.02, 0.30
GAMMA_RANGE = (0.05, 4.0)


def record(line):
    """Print a figure that profiles/batchnorm_edges.txt records; with XVEC_BN_LOG set, append it to that file as well."""
    print("[bn] " + line)
    if os.environ.get("XVEC_BN_LOG"):
        with open(os.environ["XVEC_BN_LOG"], "a") as f:
            f.write(line + "\n")


def _pre(layer):
    return f"time_context_layers.{layer}."


def _context_rows(x, layer):
    return torch.cat(oracle.get_time_context(x, oracle.CONTEXTS[layer]), 2)


def relu_ref(x, p64, layer):
    """fp64: the layer in front of its BatchNorm, relu(cat(context) W^T + b) (tdnn_layer.py:28-31)."""
    pre = _pre(layer)
    return torch.relu(_context_rows(x, layer) @ p64[pre + "linear.weight"].t() + p64[pre + "linear.bias"])


def layer_ref(x, p64, layer, eps=oracle.BN_EPS):
    """fp64: oracle.tdnn_layer with a free eps (the same operations in the same order: bit-identical at eps = 1e-5)."""
    pre = _pre(layer)
    v = relu_ref(x, p64, layer)
    return (v - p64[pre + "norm.running_mean"]) / torch.sqrt(p64[pre + "norm.running_var"] + eps) * p64[pre + "norm.weight"] \
        + p64[pre + "norm.bias"]


def chain_ref(x, p64, eps=oracle.BN_EPS, upto=5):
    """fp64 outputs of layers 0 .. upto - 1, each fed the one before."""
    outs = []
    for layer in range(upto):
        x = layer_ref(x, p64, layer, eps)
        outs.append(x)
    return outs


def pooled_xvec_ref(x, p64, eps=oracle.BN_EPS):
    """fp64 pooled statistics [B, 3000] and layer-6 x-vectors (main.py:59-63, 81-94) of fixed-length x."""
    pooled = oracle.stat_pool(chain_ref(x, p64, eps)[-1])
    return pooled, pooled @ p64["segment_layer6.weight"].t() + p64["segment_layer6.bias"]


def folded(p, layer, eps=oracle.BN_EPS):
    """fp32 (scale, shift) as pack_tdnn_vec_kernel computes them: sc = gamma / sqrtf(var + eps), sh = beta - mean * sc with the
    product and the difference contracted to one fused multiply-add (hipcc's default for device code; the exact product of
    two fp32 values fits fp64, so rounding the fp64 difference once more is the fma up to double rounding)."""
    pre = _pre(layer)
    f = lambda k: p[pre + k].float()
    sc = f("norm.weight") / torch.sqrt(f("norm.running_var") + torch.tensor(eps, dtype=torch.float32))
    sh = (f("norm.bias").double() - f("norm.running_mean").double() * sc.double()).float()
    return sc, sh


def stored_domain(y, p, layer, eps=oracle.BN_EPS):
    """(r, live): the ReLU output behind a layer's fp32 output y = r * scale + shift, in fp64, and the channels where it can be
    recovered (|scale| >= SCALE_GUARD).  Plain bf16 stores exactly r, rounded to bf16; behind the BatchNorm a bf16 step of r is
    |scale| 2^-8 r next to a y that may have cancelled to anything, so kernel-against-kernel comparisons belong here."""
    sc, sh = folded(p, layer, eps)
    live = sc.abs() >= SCALE_GUARD
    sc64 = torch.where(live, sc, torch.ones_like(sc)).double().to(y.device)
    return (y.double() - sh.double().to(y.device)) / sc64, live


# ------------------------------------------------------------------------------------------------------- the generator
def calibrated_state_dict(sd, seed, eps=oracle.BN_EPS, **arch):
    """(sd', info): a checkpoint-like copy of `sd` (tensors keyed as the reference's state_dict; `arch` are the constructor
    arguments it was made with, of which only input_size is needed and checked), calibrated layer by layer with the fp64
    oracle on synth.make_mfcc(8, 120, seed):

      * 2 % of a layer's channels are DEAD: their bias is pushed down until the largest pre-activation of the calibration
        batch is -1, so the ReLU output is 0 in every row;
      * a further 4 % are RARELY ON: their bias is lowered by their own 98th percentile;
      * the biases are rounded to fp32, then running_mean / running_var are the mean and the unbiased variance of the ReLU
        output over the calibration rows, rounded to fp32 -- exactly 0 and 0 on the dead channels;
      * |gamma| is log-uniform in [0.05, 4], 30 % are negative, 2 % exactly 0; in layers 1-4 two more channels have
        gamma = 1e-30 and 1e-42 (on both sides of pack_rows_kernel's |scale| < 1e-18 guard there is nothing else);
      * beta is N(0, 0.5);
      * the next layer is calibrated on this layer's fp64 output.

    info[layer] holds the channel index arrays "dead", "rare", "zero", "negative", "tiny"."""
    import xvector_amd as xa
    out = {k: v.clone() for k, v in sd.items()}
    cin = out[_pre(0) + "linear.weight"].shape[1] // len(oracle.CONTEXTS[0])
    assert arch.get("input_size", cin) == cin, (arch, cin)
    x = torch.as_tensor(xa.synth.make_mfcc(8, 120, input_size=cin, seed=seed)).double()
    info = []
    for layer in range(5):
        pre = _pre(layer)
        rng = np.random.default_rng([seed, layer])
        W = out[pre + "linear.weight"].double()
        cout = W.shape[0]
        rows = _context_rows(x, layer).reshape(-1, W.shape[1])
        z = rows @ W.t() + out[pre + "linear.bias"].double()
        order = rng.permutation(cout)
        n_dead, n_rare = max(1, round(DEAD_SHARE * cout)), max(1, round(RARE_SHARE * cout))
        dead, rare = np.sort(order[:n_dead]), np.sort(order[n_dead:n_dead + n_rare])
        b = out[pre + "linear.bias"].double()
        b[dead] -= z[:, dead].max(0).values + 1.0
        b[rare] -= torch.quantile(z[:, rare], 0.98, dim=0)
        b32 = b.float()
        out[pre + "linear.bias"] = b32
        r = torch.relu(rows @ W.t() + b32.double())
        mean, var = r.mean(0).float(), r.var(0, unbiased=True).float()
        assert (r[:, dead] == 0).all() and (mean[dead] == 0).all() and (var[dead] == 0).all()
        out[pre + "norm.running_mean"], out[pre + "norm.running_var"] = mean, var
        gamma = np.exp(rng.uniform(np.log(GAMMA_RANGE[0]), np.log(GAMMA_RANGE[1]), cout))
        negative = rng.random(cout) < NEG_SHARE
        gamma[negative] *= -1.0
        order = rng.permutation(cout)
        n_zero = max(1, round(ZERO_SHARE * cout))
        zero = np.sort(order[:n_zero])
        gamma[zero] = 0.0
        tiny = np.empty(0, dtype=np.int64)
        if layer < 4:
            alive = [c for c in order[n_zero:] if c not in set(dead.tolist())]
            tiny = np.asarray(alive[:len(TINY_GAMMAS)], dtype=np.int64)
            gamma[tiny] = TINY_GAMMAS
        out[pre + "norm.weight"] = torch.from_numpy(gamma.astype(np.float32))
        out[pre + "norm.bias"] = torch.from_numpy((0.5 * rng.standard_normal(cout)).astype(np.float32))
        g32 = out[pre + "norm.weight"]
        info.append({"dead": dead, "rare": rare, "zero": zero, "tiny": tiny,
                     "negative": np.flatnonzero((g32 < 0).numpy())})
        p64 = oracle.cast_params({k: v for k, v in out.items() if k.startswith(pre)}, torch.float64)
        x = layer_ref(x, p64, layer, eps)
    return out, info


def constant_channels(info, layer):
    """Channels whose BatchNorm output is beta whatever the input (calibration batch): dead (r = 0, mean = 0) or gamma = 0."""
    return np.union1d(info[layer]["dead"], info[layer]["zero"])


def off_on(x, p64, layer, channels, margin=0.25):
    """Those of `channels` that are off in EVERY row of this input too, with `margin` to spare in front of the ReLU (fp64): a
    dead channel is dead on the calibration batch; other data may light it."""
    pre = _pre(layer)
    ch = torch.as_tensor(np.asarray(channels), dtype=torch.long)
    z = _context_rows(x, layer) @ p64[pre + "linear.weight"][ch].t() + p64[pre + "linear.bias"][ch]
    return np.asarray(channels)[(z.reshape(-1, len(ch)).max(0).values < -margin).numpy()]


# ------------------------------------------------------------------------------------ plain bf16, restated on the CPU
def _bf16(t):
    """Round to bf16 (nearest even, from fp32 as the kernels do) and return the values as fp64."""
    return t.float().to(torch.bfloat16).double()


def first_kernel_bias(bias):
    """Layer 1's bias as tdnn_first reads it (pack.hip, patch_bias_kslots_kernel): two spare k slots of the bf16 weights hold
    bf16(b) and bf16(b - bf16(b)), the staged input 1.0 there -- the bias enters the sum as hi + lo."""
    hi = bias.float().to(torch.bfloat16).float()
    lo = (bias.float() - hi).to(torch.bfloat16).float()
    return hi.double() + lo.double()


def _deferred_layer(a, p, layer, eps, first_kernel):
    """One stored layer: a = the producing layer's stored output (bf16 values, fp64) or the bf16-rounded features -> the
    unrounded relu(z + bias') in fp32 (as fp64).  Weights bf16(fp32(W) * fp32(scale_prev)), bias' = fp32(bias + sum W *
    shift_prev) with the sum in fp64 over the fp32 values (pack.hip: pack_tdnn_weight_*_kernel, fold_bias_kernel)."""
    pre = _pre(layer)
    W, b = p[pre + "linear.weight"].float(), p[pre + "linear.bias"].float()
    taps = len(oracle.CONTEXTS[layer])
    if layer > 0:
        sc, sh = folded(p, layer - 1, eps)
        Wq = _bf16(W * sc.repeat(taps))
        bias = (b.double() + W.double() @ sh.double().repeat(taps)).float().double()
    else:
        Wq = _bf16(W)
        bias = first_kernel_bias(b) if first_kernel else b.double()
    z = _context_rows(a, layer) @ Wq.t()
    return torch.relu((z + bias).float()).double()


def unfold_input(x, p, layer, eps=oracle.BN_EPS):
    """A per-layer entry's way in (pack.hip, pack_rows_kernel): the caller's BatchNormed input of `layer` taken back through
    its producer's fold in fp32, r = (x - shift) / scale, 0 where |scale| < 1e-18; layer 0 reads the features as they are."""
    x = x.float()
    if layer == 0:
        return x
    sc, sh = folded(p, layer - 1, eps)
    live = sc.abs() >= SCALE_GUARD
    return torch.where(live, (x - sh) / torch.where(live, sc, torch.ones_like(sc)), torch.zeros_like(x))


def bf16_deferred_sim(x, p, eps=oracle.BN_EPS, upto=5, chained=True, first_kernel=False, unrounded_last=False):
    """Plain bf16's arithmetic, step by step, with fp64 sums in place of the matrix pipe's fp32 ones.  Every layer stores
    bf16(relu(z + bias')) and leaves its BatchNorm to its consumer's weights and bias (xvec_api.hip, refold).
    chained: x is the features [B, T, cin]; returns the stored outputs of layers 0 .. upto - 1 (bf16 values as fp64), each
    fed the one before -- the whole path's data flow.
    not chained: x is the BatchNormed fp32 input of layer upto - 1, as a per-layer entry gets it; returns that layer's stored
    output alone.
    first_kernel: layer 1 as tdnn_first runs it (first_kernel_bias).  unrounded_last: the last layer's relu output before
    its rounding to bf16 -- what layer 5's pooling epilogue sums."""
    p = {k: v for k, v in p.items() if v.is_floating_point()}
    if not chained:
        layer = upto - 1
        r = _deferred_layer(_bf16(unfold_input(x, p, layer, eps)), p, layer, eps, first_kernel)
        return r if unrounded_last else _bf16(r)
    outs, a = [], _bf16(x)
    for layer in range(upto):
        r = _deferred_layer(a, p, layer, eps, first_kernel)
        a = _bf16(r)
        outs.append(r if unrounded_last and layer == upto - 1 else a)
    return outs


def bf16_pooled_xvec_sim(x, p, eps=oracle.BN_EPS, first_kernel=False):
    """(pooled [B, 3000], layer-6 x-vector) of the simulation: layer 5's unrounded ReLU outputs pooled in fp64, its folded fp32
    BatchNorm applied as pool_finalize does (mean = shift + scale * mean r, std = |scale| * std r), the pooled row rounded to
    fp32, segment_layer6 in fp64."""
    r = bf16_deferred_sim(x, p, eps, 5, True, first_kernel, unrounded_last=True)[-1]
    sc, sh = folded(p, 4, eps)
    pooled = torch.cat((sh.double() + sc.double() * r.mean(1), sc.double().abs() * r.std(1)), 1).float().double()
    return pooled, pooled @ p["segment_layer6.weight"].double().t() + p["segment_layer6.bias"].double()


def fp32_folded_layer(x, p, layer, eps=oracle.BN_EPS):
    """The fp32 kernels' arithmetic on the CPU: relu(x W^T + b) in fp32, times scale, plus shift."""
    pre = _pre(layer)
    sc, sh = folded(p, layer, eps)
    v = torch.relu(_context_rows(x.float(), layer) @ p[pre + "linear.weight"].float().t() + p[pre + "linear.bias"].float())
    return v * sc + sh


def row_rel(got, ref):
    """Worst norm-wise relative error of a row of the last dimension."""
    g, r = got.double().cpu().reshape(-1, got.shape[-1]), ref.double().cpu().reshape(-1, ref.shape[-1])
    return ((g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30)).max().item()
