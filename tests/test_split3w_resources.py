"""Resource budget of the bf16_split3 pooling kernel on 384-channel tiles (csrc/tdnn_split3w.hip), compiled for gfx950 on the
CPU: one kernel in the translation unit, no scratch, no spill, at most 168 registers per wave -- twelve wave64 per block, one
block per CU: three waves per SIMD, 3 x registers <= 512 -- and the LDS the launch opts into per block (two buffers of three
8 KiB planes, the epilogue constants of 384 channels) is what the body addresses."""
import os
import re

from hipcc_support import CSRC, assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc_and_make

PLANNED_LDS = 2 * 3 * (128 * 32 * 2) + 3 * 384 * 4


@needs_hipcc_and_make
def test_split3w_kernel_resources():
    kernels = kernel_resources("tdnn_split3w.hip")
    assert len(kernel_instances(kernels, "tdnn_split3w_kernel")) == len(kernels) == 1, kernels
    r = next(iter(kernels.values()))
    assert_no_scratch(r, "tdnn_split3w_kernel", waves=3)
    regs = r["vgprs"] + r.get("agprs", 0)
    print("registers per wave", regs, r)
    assert regs <= 168 and 3 * regs <= 512, r
    assert r["lds"] == 0, r      # all of it dynamic: the size below is the launch's


@needs_hipcc_and_make
def test_split3w_lds_constant_is_the_one_the_launch_opts_into():
    """The value is tied by the compiler: the source static_asserts kS3wLdsBytes == 53760 = the two plane buffers + the constants
    of 384 channels that the body addresses (kernel_resources compiles the file, so a false assertion fails here), and the one
    constant is what the opt-in, the occupancy query and the launch pass."""
    kernel_resources("tdnn_split3w.hip")
    src = open(os.path.join(CSRC, "tdnn_split3w.hip")).read()
    assert re.search(r"static_assert\(kS3wLdsBytes == (\d+) && kS3wThreads == 768 && kCstFloat<true> \* 4 \+ 3 \* kS3wBN \* 4 == kS3wLdsBytes",
                     src).group(1) == str(PLANNED_LDS)
    assert src.count("kS3wLdsBytes)") + src.count("kS3wLdsBytes,") >= 5      # two opt-ins, the query, the launch, the assertion
    assert not re.search(r"<<<[^>]*>>>", src.replace("<<<dim3(grid), dim3(kS3wThreads), kS3wLdsBytes, s>>>", ""))
    assert PLANNED_LDS == 53760 and PLANNED_LDS <= 160 * 1024
