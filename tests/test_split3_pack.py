"""bf16_split3 (fp32 one-tap layers, csrc/tdnn_layer.hip S3 + pack.hip pack_tdnn_weight_split3_kernel) on the CPU:
  * the three-piece split x = hi + mid + lo is exact, bit for bit, on random and extreme fp32 values (a numpy restatement of
    the kernel's split3 and the packing kernel's arithmetic: round to nearest even at every bf16 conversion);
  * the packed weight planes (host restatement of the packing index map) hold every W[n, k] exactly where the kernel's
    fragment loads read it;
  * the split form's instantiations compile for gfx950 with no scratch, within 256 registers (two waves per SIMD), and the
    three planes of a chunk fit the LDS buffers the kernel already plans.
"""
import os

import numpy as np

from hipcc_support import CSRC, kernel_resources, needs_hipcc_and_make



def bf16_rn(x):
    """fp32 -> bf16 (round to nearest even), returned as fp32 values; NaN stays NaN."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), out)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rn(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rn(r1)
    r2 = (r1 - mid).astype(np.float32)
    lo = bf16_rn(r2)
    return hi, mid, lo


def _extremes():
    f = np.finfo(np.float32)
    v = [0.0, -0.0, 1.0, -1.0, f.tiny, -f.tiny, f.max, -f.max, f.eps, 1 + f.eps, 1 - f.epsneg, 3.0e38, 2.0 ** -100,
         2.0 ** 100, 1.0000001, 0.33333334, np.float32(np.pi), 2.0 ** -120 * 1.2345]
    # bf16 rounding ties (a 1 in bit 15 and nothing below), odd and even upper halves, the most and fewest set bits
    for base in (0x3F800000, 0x3F810000, 0x40490FDB, 0x7F7F0000, 0x00800000, 0x3F7FFFFF, 0x3F808000, 0x3F818000):
        for low in (0x0000, 0x8000, 0x7FFF, 0xFFFF, 0x0001, 0x8001):
            v.append(np.uint32((base & 0xFFFF0000) | low).view(np.float32))
    a = np.array(v, dtype=np.float32)
    return np.concatenate([a, -a])


def test_split_is_exact():
    rng = np.random.default_rng(7)
    rand = [rng.standard_normal(200000).astype(np.float32),
            (rng.standard_normal(200000) * 0.045).astype(np.float32),          # weights of the bench model's scale
            np.abs(rng.standard_normal(200000)).astype(np.float32) * 3,        # BN(ReLU)-like activations
            rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    x = np.concatenate(rand + [_extremes()])
    # values whose hi rounds up past fp32's max overflow to inf: not a value an activation or a weight takes
    x = x[np.isfinite(x) & (np.abs(x) <= np.float32(3.38e38))]
    hi, mid, lo = split3(x)
    for piece in (hi, mid, lo):
        assert np.array_equal(bf16_rn(piece), piece), "a piece is not a bf16 value"
    s = ((hi + mid).astype(np.float32) + lo).astype(np.float32)
    ok = s.view(np.uint32) == x.view(np.uint32)
    ok |= (x == 0) & (s == 0)
    # within 16 binades of the bottom of the normal range the lower pieces are bf16 subnormals (7 bits): the split loses at
    # most 2^-133 there, far below any product the layers form
    tiny = np.abs(x) < np.float32(2.0 ** -110)
    assert (np.abs(s[tiny].astype(np.float64) - x[tiny]) <= 2.0 ** -133).all()
    assert ok[~tiny].all(), x[~tiny][~ok[~tiny]][:8]
    # piece magnitudes: |mid| <= 2^-8 |hi|, |lo| <= 2^-8 |mid| (hence the dropped products < 2^-26 |x||w|)
    nz = (hi != 0) & ~tiny
    assert (np.abs(mid[nz]) <= np.abs(hi[nz]) * 2.0 ** -8).all()
    nzm = (mid != 0) & ~tiny
    assert (np.abs(lo[nzm]) <= np.abs(mid[nzm]) * 2.0 ** -8).all()


def test_six_products_match_fp64():
    """The six kept products of one dot product are within fp32 rounding of the exact one (K = 512, bench-like data)."""
    rng = np.random.default_rng(11)
    K = 512
    x = np.maximum(rng.standard_normal((64, K)), 0).astype(np.float32)
    w = (rng.standard_normal((32, K)) * 0.045).astype(np.float32)
    xs, ws = split3(x), split3(w)
    exact = x.astype(np.float64) @ w.astype(np.float64).T
    six = sum(xs[i].astype(np.float64) @ ws[j].astype(np.float64).T for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)))
    scale = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T
    assert (np.abs(six - exact) <= 2.0 ** -24 * scale).all()


def pack_split3_host(W, n_pad, k_pad):
    """Host restatement of pack_tdnn_weight_split3_kernel (one tap, K in natural order): bf16 values as fp32, flat."""
    cout, cin = W.shape
    Wp = np.zeros((n_pad, k_pad), np.float32)
    Wp[:cout, :cin] = W
    planes = split3(Wp)
    ksteps = k_pad // 16
    i = np.arange(n_pad * k_pad * 3)
    blk, within = i >> 9, i & 511
    lane, j = within >> 3, within & 7
    plane = blk % 3
    kb = blk // 3
    ct, ks = kb // ksteps, kb % ksteps
    n = ct * 32 + (lane & 31)
    k = ks * 16 + 8 * (lane >> 5) + j
    out = np.empty(i.shape, np.float32)
    for p in range(3):
        m = plane == p
        out[m] = planes[p][n[m], k[m]]
    return out


def test_packed_planes_where_the_kernel_reads_them():
    """The kernel's wave of column tile ct loads, for chunk c, k-step s, plane p, lane (r, h), the 8 bf16 at byte
    ct * (k_pad / 16) * 3072 + (6c + 3s + p) * 1024 + lane * 16 and feeds them as B[k = 32c + 16s + 8h + j][n = 32ct + r]."""
    rng = np.random.default_rng(3)
    cout, cin, n_pad, k_pad = 200, 96, 256, 128
    W = (rng.standard_normal((cout, cin)) * 0.05).astype(np.float32)
    W[0, :8] = [np.finfo(np.float32).tiny, 1.0000001, -3.0e-30, 65504.0, 2.0 ** -100, -0.0, 2.0 ** 60, 0.1]
    packed = pack_split3_host(W, n_pad, k_pad)
    pieces = np.zeros((3, n_pad, k_pad), np.float32)
    for ct in range(n_pad // 32):
        for c in range(k_pad // 32):
            for s in range(2):
                for p in range(3):
                    base = (ct * (k_pad // 16) * 3072 + (6 * c + 3 * s + p) * 1024) // 2
                    for lane in range(64):
                        r, h = lane & 31, lane >> 5
                        vals = packed[base + lane * 8: base + lane * 8 + 8]
                        k0 = 32 * c + 16 * s + 8 * h
                        pieces[p, 32 * ct + r, k0:k0 + 8] = vals
    assert np.array_equal(bf16_rn(pieces), pieces)
    rec = ((pieces[0] + pieces[1]).astype(np.float32) + pieces[2]).astype(np.float32)
    Wp = np.zeros((n_pad, k_pad), np.float32)
    Wp[:cout, :cin] = W
    assert np.array_equal(rec, Wp)     # (-0.0 comes back as +0.0)
    assert (pieces[:, cout:, :] == 0).all() and (pieces[:, :, cin:] == 0).all()


@needs_hipcc_and_make
def test_split3_kernel_resources():
    kernels = kernel_resources("tdnn_split3.hip")
    # tdnn_split3_kernel<POOL, STORE>: the split form of the store (layer 4) and pooling (layer 5) variants
    s3 = {k: v for k, v in kernels.items() if "tdnn_split3_kernel" in k}
    assert len(s3) == 2, list(kernels)
    for name, r in s3.items():
        assert r["scratch"] == 0 and r.get("spill", 0) == 0, (name, r)
        assert r["vgprs"] + r.get("agprs", 0) <= 256, (name, r)
        assert r["occupancy"] >= 2, (name, r)
    # LDS: the three 128 x 32 bf16 planes of a chunk (24 KiB) fit one of the kernel's two staging buffers (32 KiB), whose
    # layout and total (two buffers + the epilogue constants, two blocks per CU) are unchanged
    src = open(os.path.join(CSRC, "tdnn_layer_impl.h")).read()
    assert "constexpr int kPlaneBytes = kBM * kBK * 2;" in src
    assert "kLdsBytes = (2 * kStageFloats + kConstFloats) * 4;" in src
    plane, stage = 128 * 32 * 2, (128 + 128) * 32 * 4
    assert 3 * plane <= stage
    assert 2 * ((2 * (128 + 128) * 32 + 3 * 128) * 4) <= 160 * 1024
