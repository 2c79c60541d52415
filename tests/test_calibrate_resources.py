"""Resource budget of the calibration kernels (csrc/calib.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills, and the LDS of each and the waves per SIMD it leaves are what DESIGN.md ("Score
calibration") states in its table, row by row."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

WORDS = 4 * 8                  # the waves' sums of a block reduction: four doubles (or int64)
STACKS = 256 * (16 + 1) * 8    # the first hull level: a stack of XVEC_CALIB_HULL_CHUNK + 1 points of 8 bytes per thread
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "calib_gather_kernelILb0E": ("calib_gather_kernel<false>", 2 * WORDS, 8),
    "calib_gather_kernelILb1E": ("calib_gather_kernel<true>", 2 * WORDS, 8),
    "calib_mean_kernel": ("calib_mean_kernel", 2 * WORDS, 8),
    "calib_var_kernel": ("calib_var_kernel", WORDS, 8),
    "calib_start_kernel": ("calib_start_kernel", WORDS, 8),
    "calib_pass_kernel": ("calib_pass_kernel", WORDS, 4),
    "calib_solve_kernel": ("calib_solve_kernel", WORDS, 8),
    "calib_finish_kernel": ("calib_finish_kernel", 0, 8),
    "calib_apply_kernel": ("calib_apply_kernel", 0, 8),
    "calib_cllr_kernelILb0E": ("calib_cllr_kernel<false>", 2 * WORDS, 6),
    "calib_cllr_kernelILb1E": ("calib_cllr_kernel<true>", 2 * WORDS, 5),
    "calib_cllr_final_kernel": ("calib_cllr_final_kernel", 2 * WORDS, 7),
    "calib_pav_counts_kernel": ("calib_pav_counts_kernel", 16, 8),
    "calib_pav_scan_kernel": ("calib_pav_scan_kernel", 16, 8),
    "calib_hull_first_kernel": ("calib_hull_first_kernel", STACKS + 16, 4),
    "calib_hull_level_kernel": ("calib_hull_level_kernel", 0, 8),
    "calib_hull_final_kernel": ("calib_hull_final_kernel", 256 * 4 + WORDS + 8, 5),
}


@needs_hipcc
def test_calib_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("calib.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*Score calibration", design, re.M).start():]
    section = section[: section.index("\n## ", 4)]
    for want, (shown, lds, occupancy) in KERNELS.items():
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] == lds and r["occupancy"] == occupancy, (want, r)
        # DESIGN.md's table row: | `<kernel>` | <LDS bytes> | <waves per SIMD> | ...
        row = re.search(rf"\|\s*`{re.escape(shown)}`\s*\|\s*([\d,]+)\s*\|\s*(\d+)\s*\|", section)
        assert row, f"DESIGN.md does not list {shown}"
        assert int(row.group(1).replace(",", "")) == lds and int(row.group(2)) == occupancy, (want, row.group(0))
    assert 160 * 1024 // (STACKS + 16) >= 4          # the stacks leave room for the four blocks a CU's 16 wave slots of 4 hold
