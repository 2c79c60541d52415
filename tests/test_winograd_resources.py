"""Resource budget of the Winograd F(2,3) kernel (csrc/tdnn_wino.hip), compiled for gfx950 on the CPU: no scratch, at most
256 registers (two waves per SIMD: two blocks of four wave64 per CU), and the LDS it plans per block -- two staging buffers
of (64 pairs + 128 channels) x 32 floats, the block's epilogue constants and two 64-pair row tables -- small enough for the
two blocks per CU."""
import os

from hipcc_support import CSRC, assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc_and_make

PLANNED_LDS = (2 * (64 + 128) * 32 + 3 * 128 + 2 * 2 * 64) * 4 + 2 * 8


@needs_hipcc_and_make
def test_winograd_kernel_resources():
    kernels = kernel_resources("tdnn_wino.hip")
    assert len(kernel_instances(kernels, "tdnn_wino_kernel")) == len(kernels) == 1, kernels
    r = next(iter(kernels.values()))
    assert_no_scratch(r, "tdnn_wino_kernel", waves=2)
    assert r["vgprs"] + r.get("agprs", 0) <= 256, r
    # dynamic LDS: the launch size the kernel file declares is the planned one, and two blocks fit a CU's 160 KiB
    src = open(os.path.join(CSRC, "tdnn_wino.hip")).read()
    assert "kLdsBytes = (2 * kStage + kConst + 2 * kTbl) * 4 + 2 * 8" in src
    rows = open(os.path.join(CSRC, "tdnn_wino_rows.h")).read()
    assert "kBMP = kPairs;" in src and "kPairs = 64;" in rows and "kBN = 128;" in rows and "kConst = 3 * kBN;" in rows
    assert PLANNED_LDS == 51728 and 2 * PLANNED_LDS <= 160 * 1024
