"""PLDA training on the device at the edges of csrc/plda_train.hip: the shapes and branches tests/test_plda_train_gpu.py does
not reach.

  statistics   dim on the 64-column tile edge, the smallest legal calls, slice counts 1 / 2 / 3 with a ragged last chunk, a
               last row slice WITHOUT rows (the kernel must write zeros there), the element-wise staging path entered through
               a base pointer that is not 16-byte aligned, data with a large common offset.  test_stats_match_numpy's
               assertions at its 1e-12 bar; each case also runs by hand on NaN-filled outputs and a NaN-filled workspace
               and must give PldaStats's bits.
  E-step       xvec_plda_em_products by hand against numpy_products in np.longdouble, element by element inside the derived
               bound plda_em_ref.em_products_bound (derivation in its docstring), with `out` inside a sentinel-filled buffer
               and the workspace a window of exactly the reported size
  small fits   PldaStats.fit against plda_em_ref.plda_em at dim 24 and 37, rank 1 ... rank == dim, at the device path's 1e-8"""
import numpy as np
import pytest
import torch

import plda_em_ref as ref
from test_plda_train import EM_SHAPES, em_inputs, em_reference
from test_plda_train_gpu import DEV, _stats_ref

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def _data(n, dim, n_classes, seed):
    """n rows around class centres, mean about 3; every class has a row; labels shuffled."""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([np.arange(n_classes), rng.integers(0, n_classes, n - n_classes)])
    rng.shuffle(labels)
    x = 3.0 + rng.normal(0, 1, (n_classes, dim))[labels] + rng.normal(0, 1, (n, dim))
    return x, labels


def _stats_plan(n, dim):
    """(slices, rows_per_slice) of make_scatter_plan (csrc/class_scatter.h) at the 256 rows a slice of csrc/plda_train.hip, from
    the same formulas."""
    tiles = (dim + 63) // 64
    n_tri = tiles * (tiles + 1) // 2
    slices = min(max(1, 1024 // n_tri), max(1, (n + 255) // 256))
    return slices, ((n + slices - 1) // slices + 15) // 16 * 16


def _stats_by_hand(xt, labels, sf):
    """xvec_plda_stats on NaN-filled outputs and a NaN-filled workspace of the reported size: (mean, counts, sums, sums_t,
    sigma) as numpy."""
    from xvector_amd import hip, plda
    n, dim = xt.shape
    classes, order, start = plda._labels(labels, n)
    C = classes.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    mean, counts, cls, cls_t, sigma = nan(dim), nan(C), nan(C, dim), nan(dim, C), nan(dim, dim)
    wsb = int(hip.lib.xvec_plda_stats_workspace_bytes(n, dim, C))
    assert wsb > 0 and wsb % 8 == 0
    ws = nan(wsb // 8)
    order_d = torch.from_numpy(order).to(DEV)
    rc = hip.lib.xvec_plda_stats(xt.data_ptr(), hip.PLDA_X_F32 if xt.dtype == torch.float32 else hip.PLDA_X_F64, n, dim,
                                 order_d.data_ptr(), start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64)), C, sf,
                                 mean.data_ptr(), counts.data_ptr(), cls.data_ptr(), cls_t.data_ptr(), sigma.data_ptr(),
                                 ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_plda_last_error()
    return tuple(t.cpu().numpy() for t in (mean, counts, cls, cls_t, sigma))


def _check_stats(xt, x64, labels, sf, bar_mean=1e-12, bar_sigma=1e-12):
    """test_stats_match_numpy's assertions for the device tensor xt (values x64), and the poisoned run by hand."""
    from xvector_amd import plda
    st = plda.PldaStats(xt, labels, scaling_factor=sf)
    mean, sigma_obs, classes, counts, cls, raw = _stats_ref(x64, labels, sf)
    assert np.array_equal(st.classes, classes) and np.array_equal(st.counts, counts)
    assert ref.rel(st.mean, mean) <= bar_mean
    assert ref.rel(st.sigma_obs, sigma_obs) <= bar_sigma
    assert np.linalg.norm(st.class_sums() - cls) <= 1e-12 * np.linalg.norm(raw)
    assert np.array_equal(st.sigma_obs, st.sigma_obs.T)
    assert np.array_equal(st._cls_t.cpu().numpy(), st.class_sums().T)
    hand = _stats_by_hand(xt, labels, sf)
    for u, v in zip(hand, (st.mean, st.counts, st.class_sums(), st.class_sums().T, st.sigma_obs)):
        assert np.array_equal(u, v)                                          # no NaN came in from the workspace
    return st


def _on_device(x, dtype):
    x = x.astype(np.float32) if dtype == "f32" else x
    return torch.from_numpy(x).to(DEV), x.astype(np.float64)


# ---------------------------------------------------------------- statistics

@pytest.mark.parametrize("n_classes", [1, 2])
def test_stats_smallest_call(n_classes):
    """n = 2, dim = 1: one class of two rows, and every row its own class."""
    x, labels = _data(2, 1, n_classes, 3 + n_classes)
    _check_stats(*_on_device(x, "f64"), labels, 1.0)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dim", [63, 64, 65, 129])
def test_stats_at_the_tile_edge(dim, dtype):
    """dim = 65 and 129 leave a tile one column wide; 63 and 65 stage element by element, 64 by 16-byte loads."""
    x, labels = _data(300, dim, 20, dim)
    _check_stats(*_on_device(x, dtype), labels, 0.5 if dim == 65 else 1.0)


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_stats_slice_counts(n):
    """One, two and three row slices, the last chunk of the last slice ragged."""
    assert _stats_plan(n, 65)[0] == {255: 1, 256: 1, 257: 2, 513: 3}[n]
    x, labels = _data(n, 65, 9, n)
    _check_stats(*_on_device(x, "f64"), labels, 1.0)


def test_stats_last_slice_without_rows():
    """n = 7169 at dim = 512: 36 triangle tiles cap the slices at 28, 272 rows each after rounding up to 16: slice 26 holds
    97 rows, slice 27 none, and its blocks must write zero partials (the NaN-filled workspace of _check_stats shows a tile
    that was not written)."""
    n, dim = 7169, 512
    slices, rows_per_slice = _stats_plan(n, dim)
    assert (slices, rows_per_slice) == (28, 272)
    assert (slices - 1) * rows_per_slice >= n                                # the last slice starts behind the last row
    assert 0 < n - (slices - 2) * rows_per_slice < rows_per_slice            # and the one before it is ragged
    x, labels = _data(n, dim, 40, 7)
    _check_stats(*_on_device(x, "f32"), labels, 1.0)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stats_from_a_misaligned_base(dtype):
    """x starts one element into a device buffer: not 16-byte aligned, so dim % 4 == 0 stages element by element.  The
    element-wise path loads the same values into the same registers: the same sums in the same order, the same bits."""
    from xvector_amd import plda
    n, dim = 500, 64
    x, labels = _data(n, dim, 30, 11)
    fresh, x64 = _on_device(x, dtype)
    buf = torch.zeros(n * dim + 8, dtype=fresh.dtype, device=DEV)
    t = buf[1:1 + n * dim].view(n, dim)
    t.copy_(fresh)
    assert fresh.data_ptr() % 16 == 0 and t.data_ptr() % 16 != 0 and t.is_contiguous()
    a = _check_stats(t, x64, labels, 1.0)
    b = plda.PldaStats(fresh, labels)
    for u, v in ((a.mean, b.mean), (a.sigma_obs, b.sigma_obs), (a.class_sums(), b.class_sums()), (a.counts, b.counts)):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stats_with_a_large_common_offset(dtype):
    """The scatter kernel centres while it stages, so a common offset a thousand times the spread costs nothing beyond what
    float64 numpy itself loses.  The bar for mean and sigma_obs is the larger of 1e-12 and 8 x the Frobenius-relative distance
    between the float64 reference and the same statistics in np.longdouble on this input: the rounding the reference itself
    shows, with room for another summation order."""
    x, labels, _ = ref.make_data(50, 64, 8, sizes=(1, 40))
    if dtype == "f32":
        x = (x.astype(np.float32) + np.float32(1024.0)).astype(np.float32)
    else:
        x = x + 1000.0
    xt, x64 = _on_device(x, dtype)
    m64, s64 = ref.class_stats(x64, labels)[:2]
    mld, sld = ref.class_stats(x64, labels, dtype=np.longdouble)[:2]
    d_mean = float(np.linalg.norm((m64 - mld).astype(np.float64)) / np.linalg.norm(mld.astype(np.float64)))
    d_sigma = float(np.linalg.norm((s64 - sld).astype(np.float64)) / np.linalg.norm(sld.astype(np.float64)))
    st = _check_stats(xt, x64, labels, 1.0, max(1e-12, 8 * d_mean), max(1e-12, 8 * d_sigma))
    print(f"offset {dtype}: float64 vs longdouble reference: mean {d_mean:.3e}, sigma_obs {d_sigma:.3e}; "
          f"device vs float64 reference: mean {ref.rel(st.mean, m64):.3e}, sigma_obs {ref.rel(st.sigma_obs, s64):.3e}")
    assert abs(x64.mean()) > 100 * x64.std(axis=0).mean()


# ---------------------------------------------------------------- E-step products

def _window(need):
    big = torch.full((need + 8192,), GUARD, dtype=torch.uint8, device=DEV)
    off = 4096 + (-(big.data_ptr() + 4096)) % 256
    assert (big.data_ptr() + off) % 256 == 0 and off + need <= big.numel() - 2048
    big[off:off + need] = 0xFF                                               # NaN inside the window
    return big, off


@pytest.mark.parametrize("C,dim,R", EM_SHAPES)
def test_em_products_element_by_element(C, dim, R):
    """xvec_plda_em_products against numpy_products in np.longdouble, every element inside plda_em_ref.em_products_bound:
    (K + 8) 2^-53 (|A| |B|') carried through Y = S pq (K = dim), the division into H (two roundings), n H (one) and the three
    products of H (K = C) -- the derivation is the bound function's docstring.  rank == dim at (3, 5, 5) and (129, 64, 64);
    the output stride 2 R + dim is odd at (130, 37, 7); out + 2 R is the only offset C pointer xvec_gemm_nt_f64 is given."""
    from xvector_amd import hip
    sums, counts, pq_t, lam = em_inputs(C, dim, R, C + dim + R)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    sums_d, sums_t_d, counts_d, pq_d, lam_d = dev(sums), dev(sums.T), dev(counts), dev(pq_t), dev(lam)
    ldo, pad, sentinel = 2 * R + dim, 67, -12345.5
    need = int(hip.lib.xvec_plda_em_workspace_bytes(C, R))
    assert need > 0

    def call():
        buf = torch.full((R * ldo + 2 * pad,), sentinel, dtype=torch.float64, device=DEV)
        big, off = _window(need)
        rc = hip.lib.xvec_plda_em_products(pq_d.data_ptr(), sums_d.data_ptr(), sums_t_d.data_ptr(), counts_d.data_ptr(),
                                           lam_d.data_ptr(), C, dim, R, buf.data_ptr() + 8 * pad, big.data_ptr() + off, need,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, hip.lib.xvec_plda_last_error()
        torch.cuda.synchronize()
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + R * ldo:] == sentinel).all())
        assert bool((big[:off] == GUARD).all()) and bool((big[off + need:] == GUARD).all())
        return buf[pad:pad + R * ldo].view(R, ldo).cpu().numpy()

    out = call()
    assert np.isfinite(out).all() and not (out == sentinel).any()
    got = (out[:, :R], out[:, R:2 * R], out[:, 2 * R:])
    want = em_reference(sums, counts, pq_t, lam)
    bound = ref.em_products_bound(sums, counts, pq_t.T, lam)
    worst = 0.0
    for g, w, b, name in zip(got, want, bound, ("hh", "nhh", "hs")):
        ratio = float((np.abs(g - w) / b).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    print(f"E-step C={C} dim={dim} R={R}: largest error / bound = {worst:.3f}")
    assert (np.abs(got[0] - got[0].T) <= bound[0] + bound[0].T).all()        # H'H is symmetric to rounding
    assert np.array_equal(call(), out)                                       # a second call: the same bits


# ---------------------------------------------------------------- small fits through the device

@pytest.mark.parametrize("dim,rank_f,scaling_factor,string_labels", [(24, 1, 1.0, False), (24, 12, 0.5, True),
                                                                     (24, 24, 0.5, False), (37, 37, 1.0, False)])
def test_small_fits_match_restatement(dim, rank_f, scaling_factor, string_labels):
    """The data of test_host_em_matches_restatement (60 classes, one of exactly one row) through the device E-step."""
    from xvector_amd import plda
    x, labels, _ = ref.make_data(60, dim, 6, sizes=(1, 12), seed=rank_f)
    labels = labels.copy()
    labels[0] = 10_000
    if string_labels:
        labels = np.array(["id" + str(v) for v in labels], dtype=object)
    want = ref.plda_em(x, labels, rank_f, 10, scaling_factor)
    got = plda.PldaStats(torch.from_numpy(x).to(DEV), labels, scaling_factor=scaling_factor).fit(rank_f, 10)
    assert ref.rel(got[0], want[0]) <= 1e-8
    assert ref.rel(got[1] @ got[1].T, want[1] @ want[1].T) <= 1e-8
    assert ref.rel(got[2], want[2]) <= 1e-8
