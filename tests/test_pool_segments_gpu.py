"""xvec_stat_pool_segments (csrc/pool_segments.hip) against numpy: float64 two-pass mean / std(ddof=1) of the same fp32 (or
bf16-rounded) values, at the bar test_stat_pool_edge_cases uses (assert_parity, 1e-4).  Segment lengths around the wave count
(4) and the unroll (16), vector and element-wise variants of both element types, the guards, the grid.x range, and the
promises of the header: a channel constant inside a segment, order independence, bit-identical repeats."""
import numpy as np
import pytest
import torch

from conftest import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = [1, 2, 3, 4, 5, 15, 16, 17, 29, 286]


def pool(y, segs, C, rows=None, ldy=None, scale=None, shift=None, out=None):
    """y: device tensor [rows, ldy] fp32 / bf16 (or a flat view whose data_ptr is the base); segs: [(row0, n)]."""
    from xvector_amd import hip
    from xvector_amd._device import stream
    elem = 1 if y.dtype == torch.bfloat16 else 0
    rows = y.shape[0] if rows is None else rows
    ldy = y.shape[1] if ldy is None else ldy
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    r0 = torch.from_numpy(segs[:, 0].copy()).to(DEV)
    n = torch.from_numpy(segs[:, 1].astype(np.int32)).to(DEV)
    if out is None:
        out = torch.full((len(segs), 2 * C), 7.0, device=DEV)
    hip.check(hip.lib.xvec_stat_pool_segments(y.data_ptr(), elem, rows, ldy, C, r0.data_ptr(), n.data_ptr(), len(segs),
                                              None if scale is None else scale.data_ptr(),
                                              None if shift is None else shift.data_ptr(), out.data_ptr(), stream(y.device)))
    torch.cuda.synchronize()
    return out


def ref_pool(y2d, segs, C, scale=None, shift=None):
    """float64 two-pass statistics of the values the kernel reads (y2d: host float64 [rows, >= C])."""
    out = np.full((len(segs), 2 * C), np.nan)
    for i, (r0, n) in enumerate(segs):
        v = y2d[r0:r0 + n, :C]
        out[i, :C] = v.mean(0)
        if n > 1:
            out[i, C:] = v.std(0, ddof=1)
    if scale is not None:
        out[:, :C] = shift + scale * out[:, :C]
        out[:, C:] = np.abs(scale) * out[:, C:]
    return out


def host64(y):
    return y.float().double().cpu().numpy()


def check(got, ref, segs, C, what):
    got = got.double().cpu().numpy()
    one = np.asarray([n == 1 for _, n in segs])
    assert np.isnan(got[one, C:]).all(), f"{what}: n == 1 must give a NaN std"
    assert_parity(got[:, :C], ref[:, :C], 1e-4, f"{what} mean")
    if (~one).any():
        assert_parity(got[~one], ref[~one], 1e-4, what)
        assert_parity(got[~one, C:], ref[~one, C:], 1e-4, f"{what} std")


def make_rows(rng, rows, ldy, C, dtype, mean=0.0):
    """[rows, ldy] allocated to exactly rows * ldy elements, NaN in the padding columns C..ldy."""
    y = torch.from_numpy((mean + rng.standard_normal((rows, ldy))).astype(np.float32)).to(DEV).to(dtype)
    y[:, C:] = float("nan")
    return y.contiguous()


def segment_list(rng, rows):
    segs = [(int(rng.integers(0, rows - n + 1)), n) for n in NS]
    segs += [(10, 20), (10, 20), (30, 17), (25, 16), (rows - 29, 29), (rows - 1, 1), (0, rows)]   # identical, adjacent, overlapping, last row
    return segs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C, ldy", [(1500, 1536), (256, 256), (260, 260), (7, 7), (4, 4)])
def test_segment_lengths_and_widths(C, ldy, dtype):
    rng = np.random.default_rng(C)
    rows = 400
    y = make_rows(rng, rows, ldy, C, dtype)
    segs = segment_list(rng, rows)
    got = pool(y, segs, C)
    check(got, ref_pool(host64(y), segs, C), segs, C, f"C={C} ldy={ldy} {dtype}")
    # n == 1: the mean is the row itself
    i = [k for k, (_, n) in enumerate(segs) if n == 1][0]
    assert torch.equal(got[i, :C], y[segs[i][0], :C].float())
    # identical segments give identical rows
    assert torch.equal(got[len(NS)], got[len(NS) + 1])
    assert torch.equal(pool(y, segs, C).view(torch.int32), got.view(torch.int32)), "two calls must be bit-identical"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_base_four_bytes_off_takes_the_element_wise_path(dtype):
    """The same values 4 bytes further on: no 16-byte load is possible, the element-wise variant must agree."""
    rng = np.random.default_rng(11)
    rows, C = 64, 256
    off = 4 // torch.empty(0, dtype=dtype).element_size()
    flat = torch.empty(rows * C + off, device=DEV, dtype=dtype)
    y = flat[off:]
    assert y.data_ptr() % 16 == 4
    from xvector_amd import hip
    elem = int(dtype == torch.bfloat16)
    assert hip.lib.xvec_stat_pool_segments_vector(y.data_ptr(), elem, C, C) == 0, "the launcher's own choice: element-wise"
    assert hip.lib.xvec_stat_pool_segments_vector(y.data_ptr() - 4, elem, C, C) == 1
    y.copy_(torch.from_numpy(rng.standard_normal(rows * C).astype(np.float32)).to(DEV))
    segs = [(0, 64), (3, 17), (63, 1), (40, 24), (5, 2)]
    got = pool(y, segs, C, rows=rows, ldy=C)
    ref = ref_pool(host64(y).reshape(rows, C), segs, C)
    check(got, ref, segs, C, f"misaligned {dtype}")
    aligned = pool(y.clone().reshape(rows, C), segs, C)
    check(aligned, ref, segs, C, f"aligned {dtype}")


def test_seventy_thousand_segments():
    """More segments than grid.y could hold: they go on grid.x."""
    rng = np.random.default_rng(3)
    n_seg, C = 70000, 4
    y = make_rows(rng, n_seg + 1, C, C, torch.float32)
    segs = [(i, 2) for i in range(n_seg)]
    got = pool(y, segs, C).double().cpu().numpy()
    h = host64(y)
    a, b = h[:-1], h[1:]
    ref = np.concatenate([(a + b) / 2, np.abs(a - b) / np.sqrt(2.0)], 1)
    assert_parity(got, ref, 1e-4, "70000 segments")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guards_give_nan_rows_and_spare_the_neighbours(dtype):
    rng = np.random.default_rng(4)
    rows, C = 50, 260
    y = make_rows(rng, rows, 264, C, dtype)
    segs = [(0, 20), (5, 0), (10, 30), (-1, 10), (30, 20), (rows - 9, 10), (1, 49), (3, -2), (2 ** 40, 5), (49, 1)]
    bad = [1, 3, 5, 7, 8]
    got = pool(y, segs, C)
    assert torch.isnan(got[bad]).all(), "an empty segment or one outside [0, rows) gives a NaN row"
    good = [i for i in range(len(segs)) if i not in bad]
    gs = [segs[i] for i in good]
    check(got[good], ref_pool(host64(y), gs, C), gs, C, f"neighbours of guarded segments {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_channel_constant_inside_a_segment_is_exact(dtype):
    """The pivot of a segment's sums is its OWN first row: every deviation of a constant channel is exactly 0."""
    rng = np.random.default_rng(6)
    rows, C = 120, 1500
    y = make_rows(rng, rows, 1536, C, dtype, mean=50.0)
    const = float(torch.tensor(1234.5, dtype=dtype).float())      # as the element type holds it
    segs = [(20, 61), (40, 2), (79, 1), (33, 16)]
    chans = [0, 3, 777, 1499]
    y[20:81, chans] = const
    got = pool(y, segs, C)
    for i, (r0, n) in enumerate(segs):
        assert (got[i, chans] == const).all(), (i, got[i, chans].tolist())
        if n > 1:
            assert (got[i, [C + c for c in chans]] == 0.0).all(), (i, got[i, [C + c for c in chans]].tolist())
    # ... and a segment reaching outside sees the channel vary
    out = pool(y, [(10, 61)], C)
    assert (out[0, [C + c for c in chans]] > 1.0).all()
    if dtype == torch.bfloat16:      # with the affine map: |scale| * 0 is still exactly 0
        sc = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(DEV)
        sh = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(DEV)
        g2 = pool(y, segs[:2], C, scale=sc, shift=sh)
        assert (g2[:, [C + c for c in chans]] == 0.0).all()


def test_bf16_rows_with_a_deferred_affine_map():
    """scale negative in some channels, zero in others: mean = shift + scale * mean_r, std = |scale| * std_r."""
    rng = np.random.default_rng(7)
    rows, C = 300, 1500
    y = make_rows(rng, rows, 1536, C, torch.bfloat16, mean=0.5).clamp_min(0)      # like a ReLU output
    y[:, C:] = float("nan")
    sc = rng.standard_normal(C).astype(np.float32)
    sc[::7] = 0.0
    sc[1::7] = -np.abs(sc[1::7]) - 0.1
    sh = rng.standard_normal(C).astype(np.float32)
    segs = [(0, 300), (14, 286), (100, 29), (250, 5), (7, 1)]
    got = pool(y, segs, C, scale=torch.from_numpy(sc).to(DEV), shift=torch.from_numpy(sh).to(DEV))
    ref = ref_pool(host64(y), segs, C, sc.astype(np.float64), sh.astype(np.float64))
    check(got, ref, segs, C, "bf16 with scale / shift")
    g = got.cpu().numpy()
    assert (g[:, :C][:, ::7] == sh[::7]).all() and (g[:4, C:][:, ::7] == 0).all()
    assert (g[:4, C:] >= 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_large_mean_small_std(dtype):
    """mean = 1e4, std = 1 (bf16: the rounded values, steps of 64): sums of deviations about a row of the segment do not cancel."""
    rng = np.random.default_rng(8)
    rows, C = 300, 256
    y = make_rows(rng, rows, C, C, dtype, mean=1e4)
    segs = [(0, 300), (14, 286), (100, 17), (9, 2)]
    check(pool(y, segs, C), ref_pool(host64(y), segs, C), segs, C, f"|mean| >> std {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_permuting_the_segments_permutes_the_rows(dtype):
    rng = np.random.default_rng(9)
    rows, C = 400, 1500
    y = make_rows(rng, rows, 1536, C, dtype)
    segs = segment_list(rng, rows)
    got = pool(y, segs, C)
    perm = rng.permutation(len(segs))
    again = pool(y, [segs[i] for i in perm], C)
    assert torch.equal(again.view(torch.int32), got[torch.from_numpy(perm).to(DEV)].view(torch.int32))
    alone = pool(y, [segs[5]], C)
    assert torch.equal(alone.view(torch.int32), got[5:6].view(torch.int32)), "a row depends on no other segment"
