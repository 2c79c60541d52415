"""Resource budget of the bf16_split3 kernel of fp32 layers 4-5 (csrc/tdnn_split3.hip), compiled for gfx950 on the CPU, for
three blocks of four wave64 per CU, i.e. three waves per SIMD: both instantiations (store: layer 4, pooling: layer 5) without
scratch or spills, at most 168 registers (512 / 3, in the allocation granule of 8), the occupancy hipcc derives from them at
least 3, and an LDS size -- static plus the dynamic size the launch opts into, kS3LdsBytes of csrc/tdnn_layer_impl.h: two
buffers of three 8 KiB planes and the 1.5 KiB constants table -- of which three fit the CU's 160 KiB."""
import os

from hipcc_support import CSRC, assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc_and_make

PLANNED_LDS = 2 * 3 * (128 * 32 * 2) + 3 * 128 * 4


@needs_hipcc_and_make
def test_split3_kernel_holds_three_blocks_per_cu():
    kernels = kernel_resources("tdnn_split3.hip")
    assert len(kernel_instances(kernels, "tdnn_split3_kernel")) == len(kernels) == 2, kernels
    # dynamic LDS: the size the kernel file launches with is the planned one
    impl = open(os.path.join(CSRC, "tdnn_layer_impl.h")).read()
    assert "kBM = 128, kBN = 128;" in impl and "kConstFloats = 3 * kBN;" in impl and "kPlaneBytes = kBM * kBK * 2;" in impl
    assert "kS3BufBytes = 3 * kPlaneBytes;" in impl and "kS3LdsBytes = 2 * kS3BufBytes + kConstFloats * 4;" in impl
    assert "constexpr int kBK = 32;" in open(os.path.join(CSRC, "xvec_internal.h")).read()
    assert PLANNED_LDS == 50688
    src = open(os.path.join(CSRC, "tdnn_split3.hip")).read()
    assert src.count("kS3LdsBytes)") >= 3 and "kLdsBytes" not in src.replace("kS3LdsBytes", "")    # both launches, and the query
    for name, r in kernels.items():
        print(name, r)
        assert_no_scratch(r, name, waves=3)
        assert r["vgprs"] + r.get("agprs", 0) <= 168, (name, r)
        assert 3 * (r.get("lds", 0) + PLANNED_LDS) <= 160 * 1024, (name, r)
