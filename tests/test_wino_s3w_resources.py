"""Resource budget of the Winograd split3 kernel on 256-channel tiles (csrc/tdnn_wino_s3w.hip), compiled for gfx950 on the
CPU: one kernel in the translation unit, no scratch, no spill, at most 256 registers per wave -- eight wave64 per block, one
block per CU: two waves per SIMD, 2 x registers <= 512 -- and the LDS it declares per block (the four-wave kernel's two
buffers and row tables, the epilogue constants of 256 channels) within the CU's 160 KiB."""
import os

from hipcc_support import CSRC, assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc_and_make

PLANNED_LDS = 2 * (4 * 3 * 64 * 16 * 2) + 3 * 256 * 4 + 2 * 2 * 64 * 4 + 2 * 8


@needs_hipcc_and_make
def test_wino_s3w_kernel_resources():
    kernels = kernel_resources("tdnn_wino_s3w.hip")
    assert len(kernel_instances(kernels, "tdnn_wino_s3w_kernel")) == len(kernels) == 1, kernels
    r = next(iter(kernels.values()))
    assert_no_scratch(r, "tdnn_wino_s3w_kernel", waves=2)
    regs = r["vgprs"] + r.get("agprs", 0)
    print("registers per wave", regs, r)
    assert regs <= 256 and 2 * regs <= 512, r
    src = open(os.path.join(CSRC, "tdnn_wino_s3w.hip")).read()
    assert "kS3wLdsBytes = 2 * kS3Stage + 3 * kS3wBN * 4 + 2 * kTbl * 4 + 2 * 8" in src and "kS3wBN = 256;" in src
    assert "__launch_bounds__(512, 1) void tdnn_wino_s3w_kernel" in src
    assert PLANNED_LDS == 53264 and PLANNED_LDS <= 160 * 1024
