"""CPU-only checks of embedding conditioning (include/xvec_lda.h, xvector_amd.lda): the host eigenproblem against the
speechbrain-shaped route of tests/lda_ref.py, the composition of EmbeddingTransform's stages, its pickle round trip, the
argument checks of the two library calls (none of them touches a device) and the package's exports."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import lda_ref as ref
from conftest import ROOT
from hipcc_support import header_constants

# (N, D, C, rank, offset): tests/lda_ref.make_case, default_rng(1234)
CASES = [(200, 24, 7, 6, 0.0), (400, 65, 12, 8, 0.0), (300, 130, 9, 8, 1e3), (97, 17, 5, 4, 0.0)]


def test_package_exports_the_lda_surface():
    import xvector_amd as xa
    for name in ("lda", "LDA", "LdaStats", "EmbeddingTransform"):
        assert name in xa.__all__
        assert callable(getattr(xa, name)), name
    from xvector_amd import plda
    assert callable(plda.lda)                     # the drop-in for plda_classifier.lda sits next to setup_plda / train_plda
    for name in ("get_mean_stat1", "get_total_covariance_stat1", "center_stat1", "rotate_stat1", "norm_stat1", "whiten_stat1",
                 "get_lda_matrix_stat1"):
        assert callable(getattr(plda.StatObject, name)), name


def test_binding_constants_are_the_headers():
    from xvector_amd import hip
    from xvector_amd.lda import NORM_CLIP
    src = open(os.path.join(ROOT, "include", "xvec_lda.h")).read()
    embed = header_constants("xvec_lda.h", "XVEC_EMBED_")
    assert (hip.EMBED_MAX_DIM, hip.EMBED_ROW_GROUP) == (embed["MAX_DIM"], embed["ROW_GROUP"])
    assert hip.EMBED_MAX_DIM >= 3000                          # the pooled statistics must fit
    assert re.search(r"XVEC_LDA_X_F32 = (\d), XVEC_LDA_X_F64 = (\d)", src).groups() == (str(hip.LDA_X_F32), str(hip.LDA_X_F64))
    assert NORM_CLIP == ref.NORM_CLIP == 1e-8


@pytest.mark.parametrize("n,dim,n_classes,rank,offset", CASES)
def test_lda_matrix_matches_the_eig_route(n, dim, n_classes, rank, offset):
    """lda_matrix_from_scatter (eigh(Sb, Sw)) against eig(inv(Sw) @ Sb), column by column after the sign rule, at 1e-9: the
    project's bar for fp64 back ends against their restatements (the two routes agree to <= 3e-14 on these cases, with no
    imaginary parts)."""
    from xvector_amd.lda import lda_matrix_from_scatter
    x, lab = ref.make_case(n, dim, n_classes, offset)
    _, _, sw, sb, _ = ref.lda_stats(x, lab)
    want, imag = ref.lda_matrix_eig(sw, sb, rank)
    got = lda_matrix_from_scatter(sw, sb, rank)
    assert imag == 0.0
    assert got.shape == (dim, rank) and got.dtype == np.float64
    for k in range(rank):
        d = float(np.abs(got[:, k] - want[:, k]).max())
        assert d <= 1e-9, (k, d)
    assert np.allclose(np.linalg.norm(got, axis=0), 1.0, rtol=0, atol=1e-14)
    assert (got[np.abs(got).argmax(0), np.arange(rank)] > 0).all()


def test_rank_outside_its_range_raises():
    from xvector_amd.lda import LdaStats, lda_matrix_from_scatter
    x, lab = ref.make_case(97, 17, 5, 0.0)
    _, _, sw, sb, _ = ref.lda_stats(x, lab)
    for rank in (0, 18, -1):
        with pytest.raises(ValueError):
            lda_matrix_from_scatter(sw, sb, rank)
    st = LdaStats.__new__(LdaStats)               # the statistics without the device pass: matrix() is host only
    st.dim, st.n_classes, st.s_within, st.s_between = 17, 5, sw, sb
    assert st.matrix(4).shape == (17, 4)
    for rank in (0, 5, 17):                       # beyond C - 1 = 4 the eigenvalues are zero
        with pytest.raises(ValueError):
            st.matrix(rank)
    st.dim, st.n_classes = 3, 9                   # and never more than dim
    st.s_within, st.s_between = sw[:3, :3], sb[:3, :3]
    assert st.matrix(3).shape == (3, 3)
    with pytest.raises(ValueError):
        st.matrix(4)


def _apply_numpy(launches, x):
    for mean, w, normalize in launches:
        x = ref.transform(x, mean, w, normalize)
    return x


def test_stage_composition_matches_the_stages_one_by_one():
    from xvector_amd.lda import EmbeddingTransform as ET
    rng = np.random.default_rng(5)
    x = rng.normal(2.0, 1.0, (40, 12))
    mu, mu2 = rng.normal(size=12), rng.normal(size=12)
    sigma = np.cov(x.T)
    R = rng.normal(size=(12, 5))
    R2 = rng.normal(size=(5, 3))
    diag = rng.uniform(0.5, 2.0, 3)
    # centre -> centre -> whiten (no mean) -> LDA -> length norm: one launch
    t = ET([ET.center(mu), ET.center(mu2), ET.whiten(None, sigma), ET.lda(R), ET.length_norm()])
    assert len(t.launches) == 1 and t.launches[0][2] is True
    want = ref.norm_rows((x - mu - mu2) @ ref.whitening_matrix(sigma) @ R)
    assert np.abs(_apply_numpy(t.launches, x) - want).max() <= 1e-12 * np.abs(want).max()
    # a second chain behind the norm, a centre behind a rotation (a launch of its own), a diagonal whitening, a bare norm
    t = ET([ET.center(mu), ET.rotate(R), ET.length_norm(), ET.rotate(R2), ET.whiten(np.ones(3), diag), ET.length_norm(),
            ET.length_norm()])
    assert [(m is not None, w is not None, n) for m, w, n in t.launches] == [(True, True, True), (False, True, False),
                                                                             (True, True, True), (False, False, True)]
    y = ref.norm_rows((x - mu) @ R) @ R2
    want = ref.norm_rows(ref.norm_rows((y - 1.0) / np.sqrt(diag)))
    assert np.abs(_apply_numpy(t.launches, x) - want).max() <= 1e-12
    assert ET([]).launches == []
    with pytest.raises(ValueError):
        ET([ET.rotate(R), ET.rotate(R)])          # 5 columns into a 12-row rotation
    with pytest.raises(ValueError):
        ET([("scale", 2.0)])


def test_pickle_round_trip():
    from xvector_amd.lda import EmbeddingTransform as ET
    rng = np.random.default_rng(6)
    t = ET([ET.center(rng.normal(size=8)), ET.lda(rng.normal(size=(8, 3))), ET.length_norm()])
    t._dev = ["not picklable state must not travel", lambda: None]
    u = pickle.loads(pickle.dumps(t))
    assert u.device == t.device and u._dev is None and len(u.launches) == 1
    for a, b in zip(u.launches[0][:2], t.launches[0][:2]):
        assert np.array_equal(a, b)
    assert u.launches[0][2] is True


# ---------------------------------------------------------------- argument checks of the library, no device

def _err(hip):
    return hip.lib.xvec_lda_last_error().decode()


def test_stats_argument_errors_without_gpu():
    from xvector_amd import hip
    L = hip.lib
    start = (ctypes.c_int64 * 4)(0, 2, 3, 5)
    buf = ctypes.create_string_buffer(64)         # stands in for every device pointer: no check dereferences one
    p = ctypes.addressof(buf)
    need = L.xvec_lda_stats_workspace_bytes(5, 3, 3)
    assert need > 0 and need % 256 == 0
    assert L.xvec_lda_stats_workspace_bytes(0, 3, 3) == 0 and L.xvec_lda_stats_workspace_bytes(2, 3, 3) == 0
    assert L.xvec_lda_stats_workspace_bytes(5, 0, 3) == 0

    def call(x=p, dtype=1, n=5, dim=3, order=p, cs=start, C=3, mean=p, cm=p, sw=p, sb=p, ws=p, wsb=need):
        return L.xvec_lda_stats(x, dtype, n, dim, order, cs, C, mean, cm, sw, sb, ws, wsb, None)

    for kw in (dict(x=None), dict(order=None), dict(cs=None), dict(mean=None), dict(cm=None), dict(sw=None), dict(sb=None),
               dict(ws=None)):
        assert call(**kw) == hip.ERR_ARG and "null" in _err(hip), kw
    assert call(dtype=2) == hip.ERR_ARG and "x_dtype" in _err(hip)
    assert call(n=0) == hip.ERR_ARG and _err(hip)
    assert call(n=1 << 31) == hip.ERR_TOO_LARGE and "int32" in _err(hip)
    assert call(dim=0) == hip.ERR_ARG and _err(hip)
    assert call(n=2) == hip.ERR_ARG and "classes" in _err(hip)
    assert call(cs=(ctypes.c_int64 * 4)(0, 2, 2, 5)) == hip.ERR_ARG and "class 1 is empty" in _err(hip)      # an empty class
    assert call(cs=(ctypes.c_int64 * 4)(0, 3, 2, 5)) == hip.ERR_ARG and "class 1" in _err(hip)               # decreasing
    assert call(cs=(ctypes.c_int64 * 4)(1, 2, 3, 5)) == hip.ERR_ARG and "0 to n" in _err(hip)
    assert call(cs=(ctypes.c_int64 * 4)(0, 2, 3, 4)) == hip.ERR_ARG and "0 to n" in _err(hip)
    assert call(wsb=need - 1) == hip.ERR_WORKSPACE and "workspace too small" in _err(hip)


def test_transform_argument_errors_without_gpu():
    from xvector_amd import hip
    L = hip.lib
    buf = ctypes.create_string_buffer(4096)
    x, y = ctypes.addressof(buf), ctypes.addressof(buf) + 2048          # 5 x 6 doubles = 240 bytes each: apart
    need = L.xvec_embed_transform_workspace_bytes(5, 6, 4)
    assert need > 0 and need % 256 == 0
    for bad in ((0, 6, 4), (5, 0, 1), (5, 6, 0), (5, 6, 7), (5, hip.EMBED_MAX_DIM + 1, 4)):
        assert L.xvec_embed_transform_workspace_bytes(*bad) == 0, bad
    assert L.xvec_embed_transform_workspace_bytes(5, 3000, 150) > 0      # the pooled statistics
    assert L.xvec_embed_transform_workspace_bytes(5, hip.EMBED_MAX_DIM, hip.EMBED_MAX_DIM) > 0

    def call(x=x, dtype=1, n=5, dim=6, ldx=6, mean=x, w=x, rank=4, normalize=1, y=y, ldy=4, ws=x, wsb=need):
        return L.xvec_embed_transform(x, dtype, n, dim, ldx, mean, w, rank, normalize, y, ldy, ws, wsb, None)

    for kw in (dict(x=None), dict(y=None), dict(ws=None)):
        assert call(**kw) == hip.ERR_ARG and "null" in _err(hip), kw
    assert call(dtype=-1) == hip.ERR_ARG and "x_dtype" in _err(hip)
    assert call(n=0) == hip.ERR_ARG and _err(hip)
    assert call(rank=7) == hip.ERR_ARG and "rank = 7" in _err(hip)                       # rank > dim
    assert call(rank=0) == hip.ERR_ARG and "rank = 0" in _err(hip)
    assert call(dim=hip.EMBED_MAX_DIM + 1, ldx=1 << 20) == hip.ERR_TOO_LARGE and "dim" in _err(hip)
    assert call(w=None) == hip.ERR_ARG and "identity" in _err(hip)                       # w == NULL with rank != dim
    assert call(ldx=5) == hip.ERR_ARG and "strides" in _err(hip)
    assert call(ldy=3) == hip.ERR_ARG and "strides" in _err(hip)
    assert call(y=x) == hip.ERR_ARG and "overlaps" in _err(hip)                          # in place
    assert call(y=x + 5 * 6 * 8 - 8) == hip.ERR_ARG and "overlaps" in _err(hip)          # y starts in x's last element
    assert call(x=y + 5 * 4 * 8 - 8, y=y) == hip.ERR_ARG and "overlaps" in _err(hip)     # x starts in y's last element
    assert call(wsb=need - 1) == hip.ERR_WORKSPACE and "workspace too small" in _err(hip)
    assert call(wsb=0) == hip.ERR_WORKSPACE
