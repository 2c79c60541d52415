"""Waveform augmentation at the block boundaries of csrc/augment.hip: the branches tests/test_augment_gpu.py does not enter.
Everything goes through WaveAugmenter against tests/augment_ref.py with the bars test_augment_gpu.py derives (reverb_bound per
sample, 1e-14 relative on gains, 2^-23 |ref| on mixed samples, 2^-22 on normalize); no tolerance of its own.

  reverb     a block of aug_reverb_conv_kernel owns 8192 outputs and walks the taps in chunks of 16 blocks of 32: n below and
             around 32, outputs ending at 8192 / 8193, 16 / 17 tap blocks, a second block that takes the early return (a short
             response in a batch whose l_max asks for two blocks), a second block that keeps no output and only feeds max|c|,
             more taps than samples.  Every case runs a second time on a workspace filled with huge positive floats (NaN would
             be swallowed by fmaxf): a block maximum that is not written, or read from another row, changes the scale.
  mix        more than 1024 ops, so that the block's strided search for its ops takes a second step
  normalize  rows shorter than the 1024-thread block, n = 1 and 2, an all-negative row, -0.0 as the minimum
  workspace  the C ABI by hand on a window of exactly the reported size inside a 0xA5-filled buffer"""
import numpy as np
import pytest
import torch

import augment_ref as ar
from test_augment_gpu import DEV, _padded, _padding_untouched, _plan, _reverb_check, _rirs, _waves

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- reverb

def _reverb_edge(x, rirs, rir_len, idx):
    """_reverb_check (padded view, bound, status, bit-identical repeat), then the same call on a poisoned workspace."""
    from xvector_amd.augment import WaveAugmenter
    got, worst = _reverb_check(x, rirs, rir_len, idx)
    aug = WaveAugmenter(rirs=rirs, rir_len=rir_len, device=DEV)
    aug.reverb(torch.from_numpy(x).to(DEV), idx)                             # sizes the workspace
    aug._ws.fill_(0x7F)                                                      # 3.4e38 in every float
    again = aug.reverb(torch.from_numpy(x).to(DEV), idx).cpu().numpy().astype(np.float64)
    assert np.array_equal(again, got, equal_nan=True)
    assert aug.status()[1] == 0
    return got, worst


def _blocks_per_utt(n, l_max):
    return (n + l_max - 1 + 8191) // 8192


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_reverb_tiny_rows(n):
    """n around the 32-sample row of the Toeplitz product, tap counts around one and two tap blocks; h = [1] doubles exactly."""
    lens = [1, 32, 33, 64, 65]
    rirs = _rirs(lens, 40 + n)
    rirs[0, 0] = 1.0
    x = _waves(len(lens), n, 41 + n)
    assert (np.abs(x).max(axis=1) > 0).all()
    got, _ = _reverb_edge(x, rirs, lens, list(range(len(lens))))
    assert np.array_equal(got[0], 2.0 * x[0].astype(np.float64))


@pytest.mark.parametrize("n,L", [(8192, 1), (8193, 1), (8000, 193), (8000, 194)])
def test_reverb_outputs_end_at_the_block_edge(n, L):
    """n + L - 1 = 8192 (one block, full) and 8193 (a second block with one output)."""
    assert n + L - 1 in (8192, 8193) and _blocks_per_utt(n, L) == n + L - 8192
    x = _waves(2, n, 50 + L)
    _reverb_edge(x, _rirs([L], 51 + L), [L], [0, -1])


def test_reverb_tap_counts_at_the_chunk_edge():
    """481 taps are 16 tap blocks (one chunk), 482 ... 513 are 17 (a second chunk, whose staged taps end at 512 / 513):
    one batch, four responses."""
    lens = [481, 482, 512, 513]
    assert [(L + 30) // 32 + 1 for L in lens] == [16, 17, 17, 17]
    x = _waves(4, 700, 60)
    _reverb_edge(x, _rirs(lens, 61), lens, [0, 1, 2, 3])


def test_reverb_short_response_skips_its_second_block():
    """l_max = 5000 asks for two blocks per utterance; the 7-tap row has 4006 outputs, so its second block takes the early
    return and must still write a zero maximum (the poisoned rerun of _reverb_edge sees a maximum that was left alone)."""
    n, lens = 4000, [7, 5000]
    assert _blocks_per_utt(n, max(lens)) == 2 and n + lens[0] - 1 <= 8192
    x = _waves(3, n, 62)
    got, _ = _reverb_edge(x, _rirs(lens, 63), lens, [0, 1, -1])
    assert np.array_equal(got[2], x[2].astype(np.float64))


def test_reverb_peak_in_a_block_without_kept_output():
    """max|c| lies in the second block, which writes nothing to c[:n] (its first tap block is c_lo = 132 > 0)."""
    n, L = 4000, 5000
    x = np.zeros((1, n), dtype=np.float32)
    x[0, -100:] = _waves(1, 100, 64)[0]
    h = np.zeros((1, L), dtype=np.float32)
    h[0, 0], h[0, L - 1] = 0.1, 1.0
    assert np.abs(ar.conv_full(x[0], h[0])).argmax() >= 8192 > n
    assert 256 - (n - 1) // 32 > 0
    _reverb_edge(x, h, [L], [0])


def test_reverb_more_taps_than_samples():
    """n = 100, L = 9000: two blocks; the first walks all 16 chunks of its 256 tap blocks against four rows of x."""
    n, L = 100, 9000
    assert _blocks_per_utt(n, L) == 2 and min((L + 30) // 32 + 1, 256) == 16 * 16
    _reverb_edge(_waves(2, n, 65), _rirs([L], 66), [L], [0, 0])


# ---------------------------------------------------------------- mix

MIX_B, MIX_N = 1300, 96


def _many_ops():
    """1300 utterances of 96 samples, utterance u with u % 3 ops: 1299 ops, one or two sources each."""
    rng = np.random.default_rng(70)
    pool = (rng.standard_normal((5, 200)) * 3000).astype(np.int16)
    lens = np.array([200, 150, 200, 120, 200])
    for r in range(5):
        pool[r, lens[r]:] = 0
    ops, srcs = [], []
    for u in range(MIX_B):
        for _ in range(u % 3):
            length = int(rng.integers(1, MIX_N + 1))
            offset = int(rng.integers(0, MIX_N - length + 1))
            k = int(rng.integers(1, 3))
            first = len(srcs)
            for _ in range(k):
                row = int(rng.integers(0, 5))
                srcs.append((row, int(rng.integers(0, lens[row]))))
            ops.append((u, offset, length, first, k, 10 ** float(rng.uniform(0.3, 1.5))))
    return pool, lens, _plan(ops, srcs, [-1] * MIX_B), _waves(MIX_B, MIX_N, 71)


@pytest.fixture(scope="module")
def many_ops():
    pool, lens, plan, x = _many_ops()
    ref, gains = ar.mix(x, pool, lens, plan.ops, plan.srcs)
    return pool, lens, plan, x, ref, gains


def test_mix_more_ops_than_threads(many_ops):
    from xvector_amd.augment import WaveAugmenter
    pool, lens, plan, x, ref, gains = many_ops
    utt = plan.ops["utt"]
    assert len(plan.ops) > 1024                                              # the search loop takes a second step
    first = {int(u): int(np.flatnonzero(utt == u)[0]) for u in np.unique(utt)}
    assert max(first.values()) >= 1024                                       # ... and finds a first op there
    past = [int(lens[s["row"]]) < int(s["start"]) + int(op["length"]) for op in plan.ops
            for s in plan.srcs[op["first_src"]:op["first_src"] + op["n_src"]]]
    assert any(past) and not all(past)                                       # some sources end inside their op
    assert (gains > 0).all() and np.isfinite(gains).all()
    aug = WaveAugmenter(pool, lens, device=DEV)
    view, buf = _padded(x)
    got = aug.mix(view, plan, inplace=True).cpu().numpy()
    assert _padding_untouched(buf, MIX_B, MIX_N) and aug.status()[0] == 0
    g = aug.last_gains.cpu().numpy()
    rel = np.abs(g - gains) / np.abs(gains)
    print(f"mix {len(plan.ops)} ops: gains rel err {rel.max():.3e}")
    assert (rel <= 1e-14).all()
    assert (np.abs(got.astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref)).all()
    no_ops = np.setdiff1d(np.arange(MIX_B), utt)
    assert len(no_ops) > 400 and np.array_equal(got[no_ops], x[no_ops])      # rows without ops: the input's bits
    assert not np.array_equal(got[utt], x[utt])
    got32 = WaveAugmenter(pool.astype(np.float32), lens, device=DEV).mix(torch.from_numpy(x).to(DEV), plan)
    assert np.array_equal(got32.cpu().numpy(), got)                          # the same pool as fp32: the same bits
    assert np.array_equal(aug.mix(torch.from_numpy(x).to(DEV), plan).cpu().numpy(), got)


# ---------------------------------------------------------------- normalize

@pytest.mark.parametrize("n", [1, 2, 63, 1023, 1024, 1025])
def test_normalize_short_rows(n):
    from xvector_amd.augment import WaveAugmenter
    B = 300
    x = _waves(B, n, 80 + n)
    if n > 1:
        x[1] = -np.abs(x[1]) - 1.0                                           # an all-negative row
        x[2] = np.abs(x[2]) + 1.0
        x[2, n // 2] = -0.0                                                  # -0.0 is the minimum
        assert (x.max(axis=1) > x.min(axis=1)).all()
    view, buf = _padded(x)
    aug = WaveAugmenter(device=DEV)
    got = aug.normalize(view, inplace=True).cpu().numpy()
    assert _padding_untouched(buf, B, n)
    if n == 1:
        assert np.isnan(got).all()                                           # 0 / 0, as the reference
        return
    ref = ar.normalize(x)
    assert np.abs(got - ref).max() <= 2.0 ** -22
    rows = np.arange(B)
    assert (got[rows, x.argmin(axis=1)] == 0.0).all() and (got[rows, x.argmax(axis=1)] == 1.0).all()
    assert got[2, n // 2] == 0.0 and got.min() == 0.0 and got.max() == 1.0
    assert np.array_equal(aug.normalize(torch.from_numpy(x).to(DEV)).cpu().numpy(), got)


# ---------------------------------------------------------------- workspace bounds, the C ABI by hand

GUARD = 0xA5


def _window(need):
    """A device byte buffer filled with 0xA5 and the offset of a 256-byte aligned window of `need` bytes in its middle."""
    big = torch.full((need + 8192,), GUARD, dtype=torch.uint8, device=DEV)
    off = 4096 + (-(big.data_ptr() + 4096)) % 256
    assert (big.data_ptr() + off) % 256 == 0 and off + need <= big.numel() - 2048
    return big, off


def _outside_untouched(big, off, need):
    return bool((big[:off] == GUARD).all()) and bool((big[off + need:] == GUARD).all())


def test_reverb_stays_inside_its_workspace():
    from xvector_amd import hip
    from xvector_amd.augment import WaveAugmenter
    n, lens, idx = 4000, [7, 5000], [0, 1, -1]
    x, rirs = _waves(3, n, 62), _rirs(lens, 63)
    aug = WaveAugmenter(rirs=rirs, rir_len=lens, device=DEV)
    want = aug.reverb(torch.from_numpy(x).to(DEV), idx).cpu().numpy()
    need = int(hip.lib.xvec_aug_reverb_workspace_bytes(3, n, rirs.shape[1]))
    assert need > 0
    big, off = _window(need)
    waves = torch.from_numpy(x).to(DEV)
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    status = torch.zeros(2, dtype=torch.int64, device=DEV)
    rc = hip.lib.xvec_aug_reverb(waves.data_ptr(), n, 3, n, aug.rirs.data_ptr(), len(lens), rirs.shape[1],
                                 aug.rir_len.data_ptr(), idx_d.data_ptr(), status.data_ptr(), big.data_ptr() + off, need,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_aug_last_error()
    torch.cuda.synchronize()
    assert _outside_untouched(big, off, need)
    assert not bool((big[off:off + need] == GUARD).all())                    # the window was the one in use
    assert np.array_equal(waves.cpu().numpy(), want) and status.cpu().tolist() == [0, 0]


def test_mix_stays_inside_its_workspace(many_ops):
    from xvector_amd import hip
    from xvector_amd.augment import WaveAugmenter
    pool, lens, plan, x, _, _ = many_ops
    aug = WaveAugmenter(pool, lens, device=DEV)
    want = aug.mix(torch.from_numpy(x).to(DEV), plan).cpu().numpy()
    want_gains = aug.last_gains.cpu().numpy()
    n_ops = len(plan.ops)
    need = int(hip.lib.xvec_aug_mix_workspace_bytes(MIX_B, MIX_N, n_ops))
    assert need > 0
    big, off = _window(need)
    waves = torch.from_numpy(x).to(DEV)
    srcs, _ = plan.on(aug.device)
    gains = torch.empty(n_ops, dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int64, device=DEV)
    rc = hip.lib.xvec_aug_mix(waves.data_ptr(), MIX_N, MIX_B, MIX_N, aug.pool.data_ptr(), hip.AUG_POOL_I16, pool.shape[0],
                              pool.shape[1], aug.pool_len.data_ptr(), plan.ops.ctypes.data_as(hip.C.c_void_p), n_ops,
                              srcs.data_ptr(), len(plan.srcs), gains.data_ptr(), status.data_ptr(), big.data_ptr() + off, need,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_aug_last_error()
    torch.cuda.synchronize()
    assert _outside_untouched(big, off, need)
    assert not bool((big[off:off + need] == GUARD).all())
    assert np.array_equal(waves.cpu().numpy(), want) and np.array_equal(gains.cpu().numpy(), want_gains)
    assert status.cpu().tolist() == [0, 0]
