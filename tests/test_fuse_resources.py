"""Resource budget of the fusion kernels (csrc/fuse.hip), compiled for gfx950 on the CPU: every kernel of the file is there,
all eight instantiations of the multi-sum pass included; none uses scratch or spills (the up to 55 fp64 accumulators of the
pass stay in registers); and the LDS of each and the waves per SIMD it leaves are what DESIGN.md ("Score fusion") states in
its table, row by row."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

WORDS = 4 * 8                  # the waves' sums of a block reduction: four doubles (or int64)
SOLVE = 2240                   # the sums (55), H and L (81 each), g and d, the state's x, y and d (9 each), the active list, as the compiler lays them out
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "fuse_gather_kernelILb0E": ("fuse_gather_kernel<false>", 2 * WORDS, 4),
    "fuse_gather_kernelILb1E": ("fuse_gather_kernel<true>", 2 * WORDS, 4),
    "fuse_mean_kernel": ("fuse_mean_kernel", 2 * WORDS + 5 * 8 + 3 * 8 * 8, 8),
    "fuse_var_kernel": ("fuse_var_kernel", WORDS, 8),
    "fuse_start_kernel": ("fuse_start_kernel", WORDS, 8),
    "fuse_pass_kernelILi1E": ("fuse_pass_kernel<1>", WORDS, 4),
    "fuse_pass_kernelILi2E": ("fuse_pass_kernel<2>", WORDS, 3),
    "fuse_pass_kernelILi3E": ("fuse_pass_kernel<3>", WORDS, 3),
    "fuse_pass_kernelILi4E": ("fuse_pass_kernel<4>", WORDS, 3),
    "fuse_pass_kernelILi5E": ("fuse_pass_kernel<5>", WORDS, 3),
    "fuse_pass_kernelILi6E": ("fuse_pass_kernel<6>", WORDS, 2),
    "fuse_pass_kernelILi7E": ("fuse_pass_kernel<7>", WORDS, 2),
    "fuse_pass_kernelILi8E": ("fuse_pass_kernel<8>", WORDS, 2),
    "fuse_solve_kernel": ("fuse_solve_kernel", SOLVE, 8),
    "fuse_finish_kernel": ("fuse_finish_kernel", 0, 8),
    "fuse_apply_kernel": ("fuse_apply_kernel", 0, 8),
}


@needs_hipcc
def test_fuse_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("fuse.hip")
    assert len(kernels) == len(KERNELS) == 16, sorted(kernels)
    assert len(kernel_instances(kernels, "fuse_pass_kernel")) == 8
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*Score fusion", design, re.M).start():]
    section = section[: section.index("\n## ", 4)] if "\n## " in section[4:] else section
    for want, (shown, lds, occupancy) in KERNELS.items():
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r.get("agprs", 0) == 0, (want, r)              # the accumulators need no second register file either
        assert r["lds"] == lds and r["occupancy"] == occupancy, (want, r)
        # DESIGN.md's table row: | `<kernel>` | <LDS bytes> | <waves per SIMD> | ...
        row = re.search(rf"\|\s*`{re.escape(shown)}`\s*\|\s*([\d,]+)\s*\|\s*(\d+)\s*\|", section)
        assert row, f"DESIGN.md does not list {shown}"
        assert int(row.group(1).replace(",", "")) == lds and int(row.group(2)) == occupancy, (want, row.group(0))
    # the pass at K = 1 leaves what calibration's pass leaves: the same loads and sums
    calib = kernel_resources("calib.hip")
    assert kernels[kernel_instances(kernels, "fuse_pass_kernelILi1E")[0]]["occupancy"] == \
        calib[kernel_instances(calib, "calib_pass_kernel")[0]]["occupancy"]
