"""Seeded random batch shapes through the large-batch kernels (tdnn_pp16.hip, tdnn_first.hip) against the 128x128 kernels.

The persistent blocks of the large-batch kernels cut their row ranges into tiles of 2, 3 or 4 units of 64 frames, keep
per-utterance pooling segments across tiles and mask the units past a range's end; which of those paths a launch takes
depends on B, T and the utterance lengths.  The fixed shapes of test_large_batch_layers_gpu.py pin the known cases; this
file walks shapes nobody chose: every case compares layer 3's whole output, the pooled statistics and the x-vectors of
the SAME arithmetic on the two kernel families (tight: they differ by summation order only) and a repeat run bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_parity, assert_parity_masked
from tdnn_support import DEV, make_model

pytestmark = pytest.mark.gpu


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ragged = bool(i % 2)
        B = int(rng.integers(52, 420))
        T = int(rng.integers(60, 700)) if ragged else int(rng.integers(40, 520))
        if B * T > 150_000:                       # keep a case under ~1 s and 1 GB
            T = max(40, 150_000 // B)
        out.append((B, T, ragged, int(rng.integers(1 << 30))))
    return out


@pytest.fixture(scope="module")
def engines(sd42):
    return {p: (make_model(sd42, precision=p), make_model(sd42, {"XVEC_PP": "0"}, p)) for p in ("bf16", "bf16x3")}


# (FUZZ_N / FUZZ_SEED: a longer walk by hand; FUZZ_N=80 FUZZ_SEED=7 and FUZZ_N=300 FUZZ_SEED=31337 ran clean in round 3:
#  629 cases passed, the rest too small for the large-batch kernels)
@pytest.mark.parametrize("B,T,ragged,seed", _cases(int(os.environ.get("FUZZ_N", "14")), int(os.environ.get("FUZZ_SEED", "2024"))))
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_random_shapes_large_batch_vs_128x128(engines, synth, gpu_model, precision, B, T, ragged, seed):
    m_pp, m_old = engines[precision]
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(synth.make_mfcc(B, T, seed=seed % 100000)).to(DEV)
    lengths = rng.integers(max(16, T // 4), T + 1, B).tolist() if ragged else None
    if ragged:
        lengths[int(rng.integers(B))] = T            # the padded length is reached by someone
        lengths[int(rng.integers(B))] = 16           # and the shortest utterance with a defined std (two frames after 14 of context) too
    # bf16: the two kernel families round fp32 sums that differ in summation order to bf16 -- a flipped rounding (2^-8 of one
    # activation) shows at 2e-4 in the statistics of a two-frame utterance (measured), 1e-5 in those of a long one
    # (and its large-batch pooling sums bf16-rounded deviations, tdnn_pp16.hip SegMx: ~1e-4 of a statistic over 286 frames)
    tight = 2e-3 if precision == "bf16" else 2e-5
    got = m_pp.pooled(x, lengths=lengths)
    disp = m_pp.last_dispatch()
    frames = (sum(lengths) if ragged else B * T) - 14 * B
    if frames < 16000:                               # layers 2-4 switch at 1.8 units of 64 frames per CU: 14.7 k frames
        pytest.skip(f"batch too small for the large-batch kernels: {disp}")
    assert disp[1:] == ["pp"] * 4, disp
    assert torch.equal(got, m_pp.pooled(x, lengths=lengths)), "repeat run differs"
    old = m_old.pooled(x, lengths=lengths)
    assert m_old.last_dispatch()[1:] == ["tile128"] * 4
    # element-wise at the arithmetic's bar (bf16 2e-2; bf16x3's 2e-4 is the check on the kernels' logic) on every utterance with
    # at least four pooled frames; the shorter ones (one flipped bf16 rounding moves the std of a TWO-frame utterance by ~1e-2
    # of itself) are listed explicitly and checked norm-wise only
    short = torch.zeros_like(got, dtype=torch.bool)
    if ragged:
        short[torch.as_tensor([n - 14 < 4 for n in lengths])] = True
    assert_parity_masked(got, old, tight, f"{precision} pooled B={B} T={T} ragged={ragged}",
                         2e-2 if precision == "bf16" else 10 * tight, short,
                         # exactly the one 16-frame utterance of a ragged batch (profiles/r05_mask_shares.txt: 1 / B of the rows in
                         # every case of a full run); 1.5 x that, and nothing in a fixed-length batch
                         max_excluded=1.5 / B if ragged else 0.0)
    assert_parity(m_pp.extract_x_vec(x, lengths=lengths), m_old.extract_x_vec(x, lengths=lengths), tight,
                  f"{precision} x-vectors B={B} T={T} ragged={ragged}", elem_tol=10 * tight)
    # and against the exact fp32 path at the precision's own bar
    assert_parity(got, gpu_model.pooled(x, lengths=lengths), 1e-2 if precision == "bf16" else 1e-4,
                  f"{precision} pooled vs fp32", elem_tol=2e-2 if precision == "bf16" else 1e-3)
    if not ragged and T > 30:                        # one whole layer output, element by element
        h = gpu_model.time_context_layers[1](gpu_model.time_context_layers[0](x))
        a, b = m_pp.time_context_layers[2](h), m_old.time_context_layers[2](h)
        assert m_pp.last_dispatch()[2] == "pp"
        assert_parity(a, b, 1e-3 if precision == "bf16" else 2e-5, f"{precision} layer 3 B={B} T={T}",
                      elem_tol=1e-2 if precision == "bf16" else 2e-4)


@pytest.mark.parametrize("B,T,ragged,seed", _cases(10, 77))
def test_random_shapes_fp32_vs_oracle(gpu_model, sd42, synth, B, T, ragged, seed):
    """The headline arithmetic at shapes nobody chose: pooled statistics and x-vectors of sampled utterances against the
    fp64 oracle run per utterance on the un-padded slice (the reference's definition of a masked batch), at the path's bar."""
    import xvector_oracle as oracle
    from conftest import float_params
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(synth.make_mfcc(B, T, seed=seed % 100000))
    lengths = rng.integers(max(16, T // 4), T + 1, B).tolist() if ragged else None
    if ragged:
        lengths[int(rng.integers(B))] = T
        lengths[int(rng.integers(B))] = 16
    got_p = gpu_model.pooled(x.to(DEV), lengths=lengths).cpu()
    got_x = gpu_model.extract_x_vec(x.to(DEV), lengths=lengths).cpu()
    assert torch.equal(got_x, gpu_model.extract_x_vec(x.to(DEV), lengths=lengths).cpu()), "repeat run differs"
    p64 = oracle.cast_params(float_params(sd42), torch.float64)
    idx = sorted({0, B // 3, B // 2, B - 1} | ({int(np.argmin(lengths))} if ragged else set()))
    for j in idx:
        n = lengths[j] if ragged else T
        xj = x[j:j + 1, :n].double()
        ref_p = oracle.stat_pool(oracle.time_context_layers(xj, p64))
        ref_x = oracle.extract_x_vec(xj, p64)
        assert_parity(got_p[j:j + 1, :1500], ref_p[:, :1500], 1e-4, f"fp32 means utt {j} (n={n}) B={B} T={T} ragged={ragged}")
        # (element-wise on the stds: with two pooled frames std = |a - b| / sqrt 2, and a channel with a ~ b carries the fp32
        #  rounding of a and b at any relative size -- the fp32 reference against its own fp64 run too; norm-wise the bar holds)
        assert_parity(got_p[j:j + 1, 1500:], ref_p[:, 1500:], 1e-4, f"fp32 stds utt {j} (n={n})", elem_tol=1e-3 if n >= 64 else 5e-2)
        assert_parity(got_x[j:j + 1], ref_x, 1e-4, f"fp32 x-vector utt {j} (n={n})", elem_tol=1e-3)
