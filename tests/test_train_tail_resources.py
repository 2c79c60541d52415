"""Resource budget of the kernels of the training step's tail (csrc/train_tail.hip), compiled for gfx950 on the CPU: every
kernel of the file is there, none uses scratch or spills (the Adam kernel reads its block's tensor from the argument block
where it lies instead of indexing a copy), and the LDS stays within a CU's 160 KB.  Resource metadata only."""
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

GEMMS = tuple(f"tail_gemm_kernelILb{a}ELb{b}ELb{vec}E" for a, b in ((1, 1), (0, 0), (1, 0)) for vec in (0, 1))
KERNELS = GEMMS + ("tail_epilogue_kernel", "tail_colsum_kernel", "tail_pool_kernelILi4E", "tail_pool_kernelILi1E",
                   "tail_pool_bwd_kernelILi4E", "tail_pool_bwd_kernelILi1E", "tail_rowloss_kernel", "tail_loss_mean_kernel",
                   "tail_dlogits_kernel", "adam_step_kernel")
GEMM_LDS = 2 * 2 * 16 * 68 * 4


@needs_hipcc
def test_tail_kernels_use_no_scratch():
    kernels = kernel_resources("train_tail.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] <= 160 * 1024, (want, r)
    for want in GEMMS:
        r = kernels[kernel_instances(kernels, want)[0]]
        assert r["lds"] == GEMM_LDS, (want, r)
