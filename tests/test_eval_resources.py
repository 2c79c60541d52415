"""Resource budget of the trial-evaluation kernels (csrc/eval.hip), compiled for gfx950 on the CPU: every kernel of the file
is there, none uses scratch or spills, every one keeps at least four waves per SIMD, and the scatter kernel's LDS (the tile's
keys and bits, four per-wave digit tables, two digit tables) leaves room for several blocks per CU."""
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

KERNELS = ("eval_gather_kernelILb0", "eval_gather_kernelILb1", "eval_hist_kernel", "eval_scan_sums_kernel",
           "eval_scan_top_kernel", "eval_scan_apply_kernel", "eval_scatter_kernel", "eval_bit_sums_kernel",
           "eval_sweep_kernel", "eval_final_kernel")
SCATTER_LDS = 4096 * 4 + 4096 + 4 * 256 * 4 + 2 * 256 * 4 + 4 * 4


@needs_hipcc
def test_eval_kernels_use_no_scratch():
    kernels = kernel_resources("eval.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want, waves=4)
        assert r["lds"] <= SCATTER_LDS, (want, r)
    scatter = kernels[kernel_instances(kernels, "eval_scatter_kernel")[0]]
    assert scatter["lds"] == SCATTER_LDS and 4 * SCATTER_LDS <= 160 * 1024
