"""Resource budget of the Winograd F(2,3) kernel on bf16_split3 operands (csrc/tdnn_wino_s3.hip), compiled for gfx950 on the
CPU: no scratch, no spill, at most 256 registers (two blocks of four wave64 per CU), and the LDS it declares per block -- two
buffers of 4 products x 3 bf16 planes x 64 pairs x 16 k, the epilogue constants, two 64-pair row tables and their base rows --
small enough for the two blocks per CU.  And the split of the U planes (csrc/pack.hip, pack_wino_split3_kernel), restated
on the host: three bf16 pieces that carry U_k to about 2^-25 relative."""
import os

import numpy as np

from hipcc_support import CSRC, assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc_and_make

PLANNED_LDS = 2 * (4 * 3 * 64 * 16 * 2) + 3 * 128 * 4 + 2 * 2 * 64 * 4 + 2 * 8


@needs_hipcc_and_make
def test_wino_s3_kernel_resources():
    kernels = kernel_resources("tdnn_wino_s3.hip")
    assert len(kernel_instances(kernels, "tdnn_wino_s3_kernel")) == len(kernels) == 1, kernels
    r = next(iter(kernels.values()))
    assert_no_scratch(r, "tdnn_wino_s3_kernel", waves=2)
    assert r["vgprs"] + r.get("agprs", 0) <= 256, r
    src = open(os.path.join(CSRC, "tdnn_wino_s3.hip")).read()
    assert "kS3LdsBytes = 2 * kS3Stage + kS3Const + 2 * kTbl * 4 + 2 * 8" in src and "kS3Const = kConst * 4;" in src
    assert "kConst = 3 * kBN;" in open(os.path.join(CSRC, "tdnn_wino_rows.h")).read()
    assert "__launch_bounds__(256, 2) void tdnn_wino_s3_kernel" in src
    assert PLANNED_LDS == 51728 and 2 * PLANNED_LDS <= 160 * 1024


def _bf16(x):
    """Round float64 values to bf16 (8 significant bits, nearest even), returned as float64."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 256.0) / 256.0, e)


def test_u_plane_split_carries_u():
    rng = np.random.default_rng(5)
    W = (rng.standard_normal((3, 4096)) * 0.05).astype(np.float32).astype(np.float64)
    U = np.stack([W[0], 0.5 * ((W[0] + W[1]) + W[2]), 0.5 * ((W[0] - W[1]) + W[2]), W[2]])
    hi = _bf16(U)
    r1 = U - hi
    mid = _bf16(r1)
    lo = _bf16(r1 - mid)
    rel = np.abs(hi + mid + lo - U) / np.abs(U).clip(1e-30)
    assert rel.max() <= 2.0 ** -24, rel.max()
    # U_0 and U_3 are fp32 values: three pieces hold them exactly
    assert np.array_equal(hi[0] + mid[0] + lo[0], U[0]) and np.array_equal(hi[3] + mid[3] + lo[3], U[3])
