"""Resource budget of the bootstrap kernels (csrc/boot.hip), compiled for gfx950 on the CPU: every kernel of the file is there --
its own, the 32-bit instantiation of the shared scatter kernel and the sort's other kernels; none uses scratch or spills; the
LDS of each stays within what a block may declare (64 KiB) and is, with the waves per SIMD it leaves, what DESIGN.md
("Bootstrap") states in its table, row by row.  And the byte instantiation of the scatter kernel in csrc/eval.hip is still the
only one there."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

CANDS = 2 * 256 * 24           # an EerCand and a DcfCand per thread: the block's arg-min
SCATTER = 4096 * 4 + 4096 * 4 + 4 * 256 * 4 + 2 * 256 * 4 + 4 * 4      # the tile's keys and 32-bit payloads, the digit tables
BLOCK_LDS = 64 * 1024
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "boot_gather_kernelILb0ELi0E": ("boot_gather_kernel<false, order>", 16, 8),
    "boot_gather_kernelILb0ELi1E": ("boot_gather_kernel<false, groups>", 16, 8),
    "boot_gather_kernelILb0ELi2E": ("boot_gather_kernel<false, poisson>", 16, 8),
    "boot_gather_kernelILb1ELi0E": ("boot_gather_kernel<true, order>", 16, 8),
    "boot_gather_kernelILb1ELi1E": ("boot_gather_kernel<true, groups>", 16, 8),
    "boot_gather_kernelILb1ELi2E": ("boot_gather_kernel<true, poisson>", 16, 8),
    "eval_hist_kernel": ("eval_hist_kernel", 1024, 8),
    "eval_scan_sums_kernel": ("eval_scan_sums_kernel", 16, 8),
    "eval_scan_top_kernel": ("eval_scan_top_kernel", 16, 8),
    "eval_scan_apply_kernel": ("eval_scan_apply_kernel", 16, 8),
    "eval_scatter_kernelIjE": ("eval_scatter_kernel<uint32_t>", SCATTER, 4),
    "boot_counts_kernel": ("boot_counts_kernel", 16384 * 2, 5),
    "boot_tile_sums_kernelILb0E": ("boot_tile_sums_kernel<groups>", 32, 6),
    "boot_tile_sums_kernelILb1E": ("boot_tile_sums_kernel<poisson>", 32, 3),
    "boot_scan_kernel": ("boot_scan_kernel", 32, 8),
    "boot_sweep_kernelILb0E": ("boot_sweep_kernel<groups>", CANDS + 32, 2),
    "boot_sweep_kernelILb1E": ("boot_sweep_kernel<poisson>", CANDS + 32, 1),
    "boot_final_kernel": ("boot_final_kernel", CANDS, 8),
    "boot_summary_kernel": ("boot_summary_kernel", 0, 8),
}


@needs_hipcc
def test_boot_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("boot.hip")
    assert len(kernels) == len(KERNELS) == 19, sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*Bootstrap", design, re.M).start():]
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
    # several blocks of the 32-bit scatter still fit a CU's 160 KiB
    assert 4 * SCATTER <= 160 * 1024


@needs_hipcc
def test_eval_keeps_the_byte_instantiation_of_the_shared_sort():
    """csrc/eval.hip compiles the scatter kernel for its one-byte payload only, with the LDS it had: the 32-bit instantiation
    lives in boot.hip, and the two files share the sort's source (csrc/trial_sort.h)."""
    ev, bo = kernel_resources("eval.hip"), kernel_resources("boot.hip")
    byte, word = kernel_instances(ev, "eval_scatter_kernel"), kernel_instances(bo, "eval_scatter_kernel")
    assert len(byte) == 1 and "eval_scatter_kernelIhE" in byte[0] and len(word) == 1 and "eval_scatter_kernelIjE" in word[0]
    assert ev[byte[0]]["lds"] == SCATTER - 3 * 4096 and ev[byte[0]]["vgprs"] == bo[word[0]]["vgprs"]
    for shared in ("eval_hist_kernel", "eval_scan_sums_kernel", "eval_scan_top_kernel", "eval_scan_apply_kernel"):
        a, b = kernel_instances(ev, shared), kernel_instances(bo, shared)
        assert len(a) == len(b) == 1 and ev[a[0]] == bo[b[0]], shared
