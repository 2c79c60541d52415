"""Embedding conditioning on the device (csrc/lda.hip, xvector_amd.lda) against tests/lda_ref.py.

  statistics   xvec_lda_stats by hand on NaN-filled outputs, the workspace a window of exactly the reported size inside a
               guarded buffer, every element against np.longdouble inside lda_ref.lda_stats_bounds (derivation: lda_ref's
               docstring; for fp32 input the bound applies to the fp32 values as given).  dim on the 64-column tile edge and
               off the 16-byte staging path, n around the 16-row chunk and over several row slices, a class of one row, very
               unequal classes, a misaligned base, a common offset of 1e6, row slices without rows.  Both matrices == .T
               exactly, a second call gives the same bits.
  transform    xvec_embed_transform by hand against np.longdouble inside lda_ref.transform_bound: rank and dim around the
               tiles, n around the 64-row group, row strides wider than the rows on NaN-filled buffers (the padding stays
               NaN), no mean, no matrix, with and without the norm, an all-zero row, a row under the norm clip.
  end to end   lda(stat, 2), EmbeddingTransform.fit(..).apply(..) into PldaScorer.score without a host copy, and the
               StatObject methods, at 1e-9 against the restatement."""
import numpy as np
import pytest
import torch

import lda_ref as ref
from score_support import guards_intact, window

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LD = np.longdouble
NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=DEV)


def _labels_unequal(n, n_classes, rng):
    """Class 0 has exactly one row (n > n_classes), class 1 about 60 % of the rows, every class at least one; shuffled."""
    lab = np.arange(n_classes)
    if n > n_classes:
        rest = n - n_classes
        big = (rest * 3) // 5 if n_classes > 1 else rest
        others = rng.integers(min(1, n_classes - 1), n_classes, rest - big)      # never class 0 (unless it is the only one)
        lab = np.concatenate([lab, np.full(big, min(1, n_classes - 1)), others])
    rng.shuffle(lab)
    return lab


def _on_device(x, dtype):
    x = x.astype(np.float32) if dtype == "f32" else x
    return torch.from_numpy(x).to(DEV), x.astype(np.float64)


def _stats_plan(rows, dim):
    """(slices, rows_per_slice) of make_scatter_plan (csrc/class_scatter.h) at the 32 rows a slice of csrc/lda.hip, from the same
    formulas."""
    tiles = (dim + 63) // 64
    n_tri = tiles * (tiles + 1) // 2
    slices = min(max(1, 1024 // n_tri), max(1, (rows + 31) // 32))
    return slices, ((rows + slices - 1) // slices + 15) // 16 * 16


def _stats_by_hand(xt, labels):
    """(mean, class_means, s_within, s_between) of xvec_lda_stats on NaN-filled outputs inside an exact workspace window."""
    from xvector_amd import hip, plda
    n, dim = xt.shape
    classes, order, start = plda._labels(labels, n)
    C = classes.shape[0]
    outs = _nan(dim), _nan(C, dim), _nan(dim, dim), _nan(dim, dim)
    need = int(hip.lib.xvec_lda_stats_workspace_bytes(n, dim, C))
    assert need > 0
    big, off = window(need, DEV)
    order_d = torch.from_numpy(order).to(DEV)
    rc = hip.lib.xvec_lda_stats(xt.data_ptr(), hip.LDA_X_F32 if xt.dtype == torch.float32 else hip.LDA_X_F64, n, dim,
                                order_d.data_ptr(), start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64)), C,
                                *(t.data_ptr() for t in outs), big.data_ptr() + off, need,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_lda_last_error()
    torch.cuda.synchronize()
    assert guards_intact(big, off, need)
    return tuple(t.cpu().numpy() for t in outs)


def _check_stats(xt, x64, labels, rows=None):
    """Every element of the four outputs inside its bound (the matrices on `rows` only, if given), symmetry, repeatability."""
    got = _stats_by_hand(xt, labels)
    mean, cm, sw, sb = got
    for a in got:
        assert np.isfinite(a).all()
    assert np.array_equal(sw, sw.T) and np.array_equal(sb, sb.T)
    for a, b in zip(_stats_by_hand(xt, labels), got):
        assert np.array_equal(a, b)                                          # a second call: the same bits
    given = ref.lda_stats(x64, labels, dtype=LD, class_means=cm, mean=mean, rows=rows)
    want = given[:2]                     # mean and class means of x itself; the matrices of `given` around the device's means
    bounds = ref.lda_stats_bounds(x64, labels, cm, mean, rows=rows)
    sel = slice(None) if rows is None else rows
    worst = []
    for name, g, w, b in (("mean", mean, want[0], bounds[0]), ("class_means", cm, want[1], bounds[1]),
                          ("s_within", sw[sel], given[2], bounds[2]), ("s_between", sb[sel], given[3], bounds[3])):
        err = np.abs(np.asarray(g - w, dtype=np.float64))
        ratio = float((err / np.where(b > 0, b, 1.0)).max())
        worst.append(f"{name} {ratio:.3f}")
        assert (err <= b).all(), (name, ratio)
    print(f"lda stats n={xt.shape[0]} dim={xt.shape[1]} {xt.dtype}: largest error / bound: " + ", ".join(worst))
    # a class of one row: its mean is the row itself, so it adds exactly 0 to s_within
    classes, counts = np.unique(labels, return_counts=True)
    for k in np.nonzero(counts == 1)[0]:
        assert np.array_equal(cm[k], x64[np.asarray(labels) == classes[k]][0])
    return got


STATS_SHAPES = [(2, 1, 1, "f64"), (15, 3, 4, "f32"), (16, 63, 5, "f64"), (17, 64, 5, "f32"), (65, 65, 6, "f64"),
                (65, 130, 3, "f32"), (200, 64, 7, "f64"), (200, 130, 9, "f32")]


@pytest.mark.parametrize("n,dim,n_classes,dtype", STATS_SHAPES)
def test_stats_element_by_element(n, dim, n_classes, dtype):
    """dim 63 / 65 / 130 leave ragged tiles and stage element by element, 64 by 16-byte loads; n = 15 / 16 / 17 sit around the
    16-row chunk, 65 and 200 open 3 and 7 row slices with a ragged last one."""
    rng = np.random.default_rng(n * 1000 + dim)
    assert _stats_plan(n, dim)[0] == {2: 1, 15: 1, 16: 1, 17: 1, 65: 3, 200: 7}[n]
    labels = _labels_unequal(n, n_classes, rng)
    x = 3.0 + rng.normal(0, 1, (n_classes, dim))[labels] + rng.normal(0, 0.5, (n, dim))
    _check_stats(*_on_device(x, dtype), labels)


def test_stats_every_row_its_own_class():
    """n = C: every class mean is its row, s_within is exactly zero."""
    x = np.random.default_rng(3).normal(2.0, 1.0, (17, 5))
    got = _check_stats(*_on_device(x, "f64"), np.arange(17))
    assert np.array_equal(got[1], x) and not got[2].any()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stats_from_a_misaligned_base(dtype):
    """x starts one element into a device buffer: not 16-byte aligned, so dim % 4 == 0 stages element by element -- the same
    values into the same registers, the same sums in the same order, the same bits."""
    n, dim = 200, 64
    rng = np.random.default_rng(11)
    labels = _labels_unequal(n, 7, rng)
    x = rng.normal(0, 1, (7, dim))[labels] + rng.normal(0, 0.5, (n, dim))
    fresh, x64 = _on_device(x, dtype)
    buf = torch.zeros(n * dim + 8, dtype=fresh.dtype, device=DEV)
    t = buf[1:1 + n * dim].view(n, dim)
    t.copy_(fresh)
    assert fresh.data_ptr() % 16 == 0 and t.data_ptr() % 16 != 0 and t.is_contiguous()
    for a, b in zip(_check_stats(t, x64, labels), _stats_by_hand(fresh, labels)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stats_with_a_common_offset_of_1e6(dtype):
    """The rows are centred by their class mean before the product, so the offset costs s_within nothing: it is held to the
    bound of its own (small) centred products, like every other case."""
    x, labels = ref.make_case(200, 24, 7, offset=1e6)
    xt, x64 = _on_device(x, dtype)
    got = _check_stats(xt, x64, labels)
    true_sw = ref.lda_stats(x64, labels, dtype=LD)[2]
    bound = ref.lda_stats_bounds(x64, labels, got[1], got[0])[2]
    # against the EXACT class means too: the device's means are off by d <= their bound, which moves s_within by d d' per class
    d = ref.lda_stats_bounds(x64, labels, got[1], got[0])[1]
    slack = np.einsum("cj,ck->jk", d, d)
    assert (np.abs(np.asarray(got[2] - true_sw, dtype=np.float64)) <= bound + slack).all()
    assert abs(x64.mean()) > 1e5 * x64.std(axis=0).mean()


def test_stats_row_slices_without_rows():
    """n = 897 at dim = 512: 36 triangle tiles cap the slices at 28, 48 rows each after rounding up to 16 -- slice 18 holds 33
    rows, slices 19 .. 27 none, and their blocks must write zero partials (the workspace window is NaN-filled: a tile that was
    not written shows).  Rows 0, 63, 64 and 511 of the matrices against np.longdouble, all of them for finiteness and symmetry."""
    n, dim = 897, 512
    assert _stats_plan(n, dim) == (28, 48) and 18 * 48 < n <= 19 * 48
    rng = np.random.default_rng(7)
    labels = _labels_unequal(n, 40, rng)
    x = rng.normal(0, 1, (40, dim))[labels] + rng.normal(0, 0.5, (n, dim))
    _check_stats(*_on_device(x, "f32"), labels, rows=[0, 63, 64, 511])


# ---------------------------------------------------------------- transform

def _transform_by_hand(xt_buf, n, dim, ldx, mean, w, rank, normalize, ldy):
    """xvec_embed_transform on a NaN-filled y of row stride ldy inside a padded buffer; returns the [n, ldy] buffer (numpy)."""
    from xvector_amd import hip
    pad = 37
    ybuf = _nan(n * ldy + 2 * pad)
    need = int(hip.lib.xvec_embed_transform_workspace_bytes(n, dim, rank))
    assert need > 0
    big, off = window(need, DEV)
    rc = hip.lib.xvec_embed_transform(xt_buf.data_ptr(), hip.LDA_X_F32 if xt_buf.dtype == torch.float32 else hip.LDA_X_F64,
                                      n, dim, ldx, None if mean is None else mean.data_ptr(),
                                      None if w is None else w.data_ptr(), rank, normalize, ybuf.data_ptr() + 8 * pad, ldy,
                                      big.data_ptr() + off, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_lda_last_error()
    torch.cuda.synchronize()
    assert guards_intact(big, off, need)
    assert bool(torch.isnan(ybuf[:pad]).all()) and bool(torch.isnan(ybuf[pad + n * ldy:]).all())
    return ybuf[pad:pad + n * ldy].view(n, ldy).cpu().numpy()


def _check_transform(n, dim, rank, dtype, with_mean, with_w, xpad, ypad, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(1.5, 1.0, (n, dim))
    mean = rng.normal(1.5, 0.2, dim) if with_mean else None
    w = rng.normal(0, 1, (dim, rank)) if with_w else None
    if with_mean and dtype == "f64":
        x[0] = mean                                     # an all-zero centred row
        if n > 2:
            x[2] = mean + 1e-12 * rng.normal(0, 1, dim)     # a row whose norm lies under the clip
    npdt = np.float32 if dtype == "f32" else np.float64
    ldx, ldy = dim + xpad, rank + ypad
    xbuf = np.full((n, ldx), np.nan, dtype=npdt)
    xbuf[:, :dim] = x
    x64 = xbuf[:, :dim].astype(np.float64)               # the values as given
    xt = torch.from_numpy(xbuf).to(DEV)
    md = None if mean is None else torch.from_numpy(mean).to(DEV)
    wd = None if w is None else torch.from_numpy(w).to(DEV)
    for normalize in (0, 1):
        got = _transform_by_hand(xt, n, dim, ldx, md, wd, rank, normalize, ldy)
        assert np.isnan(got[:, rank:]).all()             # the padding columns stay NaN
        got = got[:, :rank]
        assert np.isfinite(got).all()
        want = ref.transform(x64, mean, w, bool(normalize), dtype=LD)
        bound = ref.transform_bound(x64, mean, w, bool(normalize))
        err = np.abs(got - want)                         # np.longdouble, as the bound
        ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
        print(f"transform n={n} dim={dim} rank={rank} {dtype} mean={with_mean} w={with_w} norm={normalize}: "
              f"largest error / bound = {ratio:.3f}")
        assert (err <= bound).all(), ratio
        again = _transform_by_hand(xt, n, dim, ldx, md, wd, rank, normalize, ldy)[:, :rank]
        assert np.array_equal(again, got)                # a second call: the same bits
        if with_mean and dtype == "f64":
            assert not got[0].any()                      # the all-zero row stays all-zero, normalised or not
            if normalize and n > 2:
                raw = ref.transform(x64[2:3], mean, w, False, dtype=LD)
                assert float(np.sqrt((raw * raw).sum())) < 1e-9
                assert np.abs(got[2] - raw[0] / LD(1e-8)).max() <= bound[2].max()
        if normalize and not (with_mean and dtype == "f64"):
            assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-14


# n around the 64-row group; rank around the 16- and 64-column tiles; dim as the statistics.  xpad = 0 with dim % 4 == 0
# takes the 16-byte loads, every other case the element-wise staging.
@pytest.mark.parametrize("n,dim,rank,dtype,with_mean,xpad,ypad", [
    (1, 1, 1, "f64", True, 0, 0), (65, 3, 2, "f32", True, 3, 5), (63, 130, 1, "f64", True, 3, 5),
    (64, 130, 2, "f32", False, 2, 1), (65, 130, 15, "f64", True, 3, 0), (65, 64, 16, "f32", True, 0, 5),
    (64, 65, 17, "f64", False, 3, 5), (63, 64, 64, "f64", True, 0, 0), (65, 130, 65, "f32", True, 2, 3),
    (64, 63, 17, "f64", True, 1, 2), (129, 64, 17, "f64", True, 4, 1)])
def test_transform_element_by_element(n, dim, rank, dtype, with_mean, xpad, ypad):
    _check_transform(n, dim, rank, dtype, with_mean, True, xpad, ypad, seed=n * 131 + dim * 7 + rank)


@pytest.mark.parametrize("n,dim,dtype,with_mean,xpad,ypad", [(65, 130, "f64", True, 3, 5), (17, 3, "f32", True, 0, 0),
                                                             (16, 64, "f32", False, 2, 3), (15, 65, "f64", False, 0, 1)])
def test_centre_and_norm_without_a_matrix(n, dim, dtype, with_mean, xpad, ypad):
    """w == NULL: rank == dim, no product; 16 rows a block."""
    _check_transform(n, dim, dim, dtype, with_mean, False, xpad, ypad, seed=n + dim)


# ---------------------------------------------------------------- end to end

def test_lda_drop_in_matches_the_restatement():
    """lda(stat, 2) on the (200, 24, 7) case: the matrix and the rotated stat1 at 1e-9 after the sign rule."""
    from xvector_amd import plda
    from xvector_amd.lda import LDA, lda
    x, labels = ref.make_case(200, 24, 7)
    _, _, sw, sb, _ = ref.lda_stats(x, labels)
    want, _ = ref.lda_matrix_eig(sw, sb, 2)
    stat = plda.get_x_vec_stat(x, labels)
    new = lda(stat, 2)
    assert new is not stat and np.array_equal(stat.stat1, x)                 # a new object; the input is untouched
    assert isinstance(new.stat1, np.ndarray) and new.stat1.dtype == np.float64 and new.stat1.shape == (200, 2)
    assert np.abs(new.stat1 - x @ want).max() <= 1e-9 * np.abs(x @ want).max()
    assert np.abs(plda.lda(stat, 2).stat1 - new.stat1).max() == 0.0
    m = LDA()
    m.do_lda(stat, reduced_dim=2)
    assert np.abs(m.transform_mat - want).max() <= 1e-9
    fixed = np.random.default_rng(0).normal(size=(24, 3))
    assert np.abs(m.do_lda(stat, transform_mat=fixed).stat1 - x @ fixed).max() <= 1e-12 * np.abs(x @ fixed).max()


@pytest.mark.parametrize("whiten", [False, True])
def test_fit_apply_score_stays_on_the_device(whiten):
    """EmbeddingTransform.fit(..).apply(x) -> PldaScorer.score, no host copy in between, against the numpy-transformed vectors
    through the same scorer at 1e-9."""
    import xvector_amd as xa
    from xvector_amd.lda import EmbeddingTransform
    x, labels = ref.make_case(200, 24, 7)
    tf = EmbeddingTransform.fit(x, labels, lda_dim=6, whiten=whiten)
    assert len(tf.launches) == 1 and tf.launches[0][2] is True        # whitening and LDA fold into one matrix
    mean, F, Sigma = xa.synth.make_plda(dim=6, rank=3, seed=5)
    scorer = xa.PldaScorer(mean, F, Sigma)
    xt = torch.from_numpy(x.astype(np.float32)).to(DEV)
    y = tf.apply(xt)
    assert y.is_cuda and y.dtype == torch.float64 and y.shape == (200, 6)
    got = scorer.score(y)
    assert got.is_cuda
    y_np = x.astype(np.float32).astype(np.float64)
    for m, w, nrm in tf.launches:
        y_np = ref.transform(y_np, m, w, nrm)
    want = scorer.score(y_np).cpu().numpy()
    assert np.abs(y.cpu().numpy() - y_np).max() <= 1e-9
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-9 * np.abs(want).max()
    # and the fitted stages are the restatement's: mean, LDA matrix of the (whitened) vectors
    if not whiten:
        mu, _, sw, sb, _ = ref.lda_stats(x, labels)
        assert np.abs(tf.launches[0][0] - mu).max() <= 1e-12
        assert np.abs(tf.launches[0][1] - ref.lda_matrix_eig(sw, sb, 6)[0]).max() <= 1e-9


def test_stat_object_methods_match_the_restatement():
    from xvector_amd import plda
    x, labels = ref.make_case(97, 17, 5)
    new = lambda: plda.get_x_vec_stat(x.copy(), labels)
    mu, _, sw, sb, _ = ref.lda_stats(x, labels)
    sigma = (x - mu).T @ (x - mu) / x.shape[0]
    st = new()
    assert np.abs(st.get_mean_stat1() - mu).max() <= 1e-12
    assert np.abs(st.get_total_covariance_stat1() - sigma).max() <= 1e-12 * np.abs(sigma).max()
    assert np.abs(st.get_lda_matrix_stat1(4) - ref.lda_matrix_eig(sw, sb, 4)[0]).max() <= 1e-9
    with pytest.raises(ValueError):
        st.get_lda_matrix_stat1(5)
    R = np.random.default_rng(2).normal(size=(17, 4))
    for call, want in ((lambda s: s.center_stat1(mu), x - mu), (lambda s: s.rotate_stat1(R), x @ R),
                       (lambda s: s.norm_stat1(), ref.norm_rows(x)),
                       (lambda s: s.whiten_stat1(mu, sigma), (x - mu) @ ref.whitening_matrix(sigma)),
                       (lambda s: s.whiten_stat1(mu, np.diag(sigma)), (x - mu) / np.sqrt(np.diag(sigma)))):
        st = new()
        call(st)
        assert isinstance(st.stat1, np.ndarray) and st.stat1.dtype == np.float64
        assert np.abs(st.stat1 - want).max() <= 1e-9 * np.abs(want).max()
    st = new()
    st.whiten_stat1(mu, sigma)
    cov = st.stat1.T @ st.stat1 / x.shape[0]
    assert np.abs(cov - np.eye(17)).max() <= 1e-9                              # whitened: the identity covariance
