"""xvec_gemm_nt_f64 by hand with the strides and bases the Python wrapper never passes (it always gives lda = ldb = K,
ldc = N and 16-byte aligned bases), against numpy float64 at test_scoring.py's F64_TOL (max-norm relative 1e-10).

A and B are views with row stride K + pad into NaN-filled buffers: a load that strays into the padding puts a NaN into C.
C is a view with ldc = N + 5 into a sentinel-filled buffer: every sentinel must survive.

Which load variant a call takes (csrc/score.hip, gemm_nt): the 16-byte loads need K, lda and ldb even and both bases 16-byte
aligned; anything else takes the 8-byte loads.  So even K with an odd lda or ldb, or with a base 8 bytes off, is the 8-byte
variant with `k + 1 < K` true to the end of the row -- the case the wrapper cannot reach.

Bit-equality between the variants of one shape IS expected and asserted: load2<VEC> only decides how the pair (k, k + 1) of
a row reaches its two registers; zero fill past K and past the last row is the same; the LDS image, the chunk order of the K
loop and the MFMA sequence do not depend on VEC, lda, ldb, ldc or the bases, and the tiling is chosen from M, N, K and the
CU count alone.  Every variant therefore adds the same products in the same order."""
import numpy as np
import pytest
import torch

from test_scoring import F64_TOL, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5


def _strided(values, ld, off):
    """values [R, K] as a view with row stride ld, `off` doubles behind a 16-byte aligned base, into a NaN-filled buffer."""
    R, K = values.shape
    buf = torch.full((off + R * ld + 2,), float("nan"), dtype=torch.float64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (R, K), (ld, 1), off)
    view.copy_(torch.from_numpy(values))
    return view, buf


def _call(a, b, lda, ldb, off_a, off_b, rv=None, cv=None, cst=0.0, scale=1.0):
    from xvector_amd import hip
    (M, K), N = a.shape, b.shape[0]
    ldc, front = N + 5, 3
    av, abuf = _strided(a, lda, off_a)
    bv, bbuf = _strided(b, ldb, off_b)
    cbuf = torch.full((front + M * ldc + 7,), SENTINEL, dtype=torch.float64, device=DEV)
    c_view = torch.as_strided(cbuf, (M, N), (ldc, 1), front)
    rv_d = None if rv is None else torch.from_numpy(rv).to(DEV)
    cv_d = None if cv is None else torch.from_numpy(cv).to(DEV)
    rc = hip.lib.xvec_gemm_nt_f64(av.data_ptr(), lda, bv.data_ptr(), ldb, M, N, K, None if rv is None else rv_d.data_ptr(),
                                  None if cv is None else cv_d.data_ptr(), cst, scale, c_view.data_ptr(), ldc,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_score_last_error()
    torch.cuda.synchronize()
    mask = torch.ones_like(cbuf, dtype=torch.bool)
    torch.as_strided(mask, (M, N), (ldc, 1), front).fill_(False)
    assert bool((cbuf[mask] == SENTINEL).all())                              # the columns between N and ldc, front and back
    got = c_view.cpu().numpy()
    assert not np.isnan(got).any()                                           # nothing of the operands' padding was read
    return got, (av.data_ptr(), bv.data_ptr())


def _variants(M, N, K, variants):
    """Every (pad_a, pad_b, off_a, off_b) of `variants`, with and without rowv / colv / cst / scale, against numpy; all
    variants bit-equal (see the module docstring)."""
    rng = np.random.default_rng(M * 1000 + N + K)
    a, b = rng.normal(0, 1, (M, K)), rng.normal(0, 1, (N, K))
    rv, cv = rng.normal(0, 1, M), rng.normal(0, 1, N)
    ref0 = a @ b.T
    ref1 = -1.5 * (ref0 + rv[:, None] + cv[None, :] + 0.25)
    first = None
    for pad_a, pad_b, off_a, off_b in variants:
        lda, ldb = K + pad_a, K + pad_b
        got1, ptrs = _call(a, b, lda, ldb, off_a, off_b, rv, cv, 0.25, -1.5)
        got0, _ = _call(a, b, lda, ldb, off_a, off_b)
        assert (ptrs[0] % 16 == 0) == (off_a % 2 == 0) and (ptrs[1] % 16 == 0) == (off_b % 2 == 0)
        assert _rel(got1, ref1) < F64_TOL, (pad_a, pad_b, off_a, off_b)
        assert _rel(got0, ref0) < F64_TOL, (pad_a, pad_b, off_a, off_b)
        if first is None:
            first = (got0, got1)
        assert np.array_equal(got0, first[0]) and np.array_equal(got1, first[1]), (pad_a, pad_b, off_a, off_b)
    return a, b, first[0]


PADS = [(0, 0, 0, 0), (2, 2, 0, 0), (3, 1, 0, 0), (1, 2, 0, 0)]              # 16-byte loads twice, then an odd lda / ldb
BASES = [(0, 0, 1, 0), (2, 2, 0, 1), (2, 0, 1, 1)]                           # even strides, a base 8 bytes off


@pytest.mark.parametrize("M,N,K", [(1, 1, 2), (65, 63, 34), (129, 127, 33), (200, 300, 512)])
def test_gemm_strided_operands(M, N, K):
    """Even K with an odd lda or ldb takes the 8-byte loads; K = 33 takes them throughout (its padding is still NaN)."""
    _variants(M, N, K, PADS)


@pytest.mark.parametrize("M,N,K", [(65, 63, 34), (200, 300, 512)])
def test_gemm_misaligned_bases(M, N, K):
    """Even K, even strides, A or B (or both) based 8 bytes off a 16-byte boundary: the 8-byte loads, the aligned call's bits."""
    _variants(M, N, K, PADS[:1] + BASES)


def test_gemm_strided_on_the_large_tiles():
    """(3601, 3500, 272) takes the 128 x 128 tiles (tests/test_scoring.py): lda = 274, ldc = 3505, and the contiguous call's
    bits through the wrapper (pad 0 against pad 2 with the 16-byte loads on both sides: the same sums in the same order)."""
    from xvector_amd import scoring
    M, N, K = 3601, 3500, 272
    a, b, got = _variants(M, N, K, [(2, 0, 0, 0)])
    assert N + 5 == 3505 and K + 2 == 274
    wrapped = scoring.gemm_nt(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    assert np.array_equal(wrapped, got)
