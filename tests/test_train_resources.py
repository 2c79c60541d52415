"""Resource budget of the training kernels (csrc/tdnn_train.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills (the context offsets are selected from the argument block, never indexed dynamically), and
the product kernel's LDS (two operands x two buffers x 16 k rows x 132 floats) leaves room for four blocks per CU with at
least two waves per SIMD.  Resource metadata only."""
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

GEMMS = tuple(f"train_gemm_kernelILi{op}ELb{vec}E" for op in (0, 1, 2) for vec in (0, 1))
KERNELS = GEMMS + ("train_slab_reduce_kernel", "train_stats_kernel", "train_stats_merge_kernel", "train_norm_kernel",
                   "train_bn_sums_kernel", "train_col_reduce_kernel", "train_dz_kernel")
GEMM_LDS = 2 * 2 * 16 * 132 * 4


@needs_hipcc
def test_train_kernels_use_no_scratch():
    kernels = kernel_resources("tdnn_train.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] <= 160 * 1024, (want, r)
    for want in GEMMS:
        r = kernels[kernel_instances(kernels, want)[0]]
        assert r["lds"] == GEMM_LDS and 4 * GEMM_LDS <= 160 * 1024, (want, r)
        assert_no_scratch(r, want, waves=2)
