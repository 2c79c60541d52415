"""Resource budget of the score-analysis kernels (csrc/analyze.hip), compiled for gfx950 on the CPU: every kernel of the file is
there; none uses scratch or spills; the LDS of each stays within what a block may declare (64 KiB) and is, with the waves per
SIMD it leaves, what DESIGN.md ("Score analysis") states in its table, row by row."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

WAVES = 4 * 8 + 4 * 8 + 4 * 16         # the wave buffers of pass 1: doubles, counts, (extreme, position) pairs
HIST = (8192 + 64) * 4                 # the histogram copies (analyze_plan.h: kHistWords)
FINAL = 2048 * 8 + 2048 * 4 + 256 * 4 + 4 * 4 + 8 + 4 + 4      # the survivors' keys and places, a digit table, wave totals, prefix and rank
BLOCK_LDS = 64 * 1024
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "analyze_pass1_kernelILb0ELb0E": ("analyze_pass1_kernel<false, false>", WAVES, 4),
    "analyze_pass1_kernelILb1ELb0E": ("analyze_pass1_kernel<true, false>", WAVES, 4),
    "analyze_pass1_kernelILb0ELb1E": ("analyze_pass1_kernel<false, true>", WAVES + HIST, 4),
    "analyze_pass1_kernelILb1ELb1E": ("analyze_pass1_kernel<true, true>", WAVES + HIST, 4),
    "analyze_merge1_kernel": ("analyze_merge1_kernel", WAVES, 4),
    "analyze_pass2_kernelILb0E": ("analyze_pass2_kernel<false>", 32, 7),
    "analyze_pass2_kernelILb1E": ("analyze_pass2_kernel<true>", 32, 7),
    "analyze_merge2_kernel": ("analyze_merge2_kernel", 32, 8),
    "analyze_digit_kernelILb0E": ("analyze_digit_kernel<false>", 2 * 256 * 4 + 8, 8),
    "analyze_digit_kernelILb1E": ("analyze_digit_kernel<true>", 2 * 256 * 4 + 8, 8),
    "analyze_walk_kernel": ("analyze_walk_kernel", 2 * 256 * 4 + 16, 8),
    "analyze_count_kernelILb0E": ("analyze_count_kernel<false>", 16, 8),
    "analyze_count_kernelILb1E": ("analyze_count_kernel<true>", 16, 8),
    "analyze_offsets_kernel": ("analyze_offsets_kernel", 16, 8),
    "analyze_write_kernelILb0E": ("analyze_write_kernel<false>", 288, 8),
    "analyze_write_kernelILb1E": ("analyze_write_kernel<true>", 288, 8),
    "analyze_final_kernel": ("analyze_final_kernel", FINAL, 6),
}


@needs_hipcc
def test_analyze_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("analyze.hip")
    assert len(kernels) == len(KERNELS) == 17, sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*Score analysis", design, re.M).start():]
    section = section[: section.index("\n## ", 4)] if "\n## " in section[4:] else section
    for want, (shown, lds, occupancy) in KERNELS.items():
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] <= BLOCK_LDS and r["lds"] == lds and r["occupancy"] == occupancy, (want, r)
        row = re.search(rf"\|\s*`{re.escape(shown)}`\s*\|\s*([\d,]+)\s*\|\s*(\d+)\s*\|", section)
        assert row, f"DESIGN.md does not list {shown}"
        assert int(row.group(1).replace(",", "")) == lds and int(row.group(2)) == occupancy, (want, row.group(0))
    # four blocks of the histogram pass fit a CU's 160 KiB: the grid's 1024 blocks are resident at once on 256 CUs
    assert 4 * (WAVES + HIST) <= 160 * 1024
