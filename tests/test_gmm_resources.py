"""Resource budget of the GMM-UBM kernels (csrc/gmm.hip), compiled for gfx950 on the CPU: every kernel of the file is there;
none uses scratch or spills; the LDS of each stays within what a block may declare (64 KiB) and is, with the waves per SIMD it
leaves, what DESIGN.md ("GMM-UBM") states in its table, row by row."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

STAGE = 2 * 2 * 16 * 80 * 8            # the two double-buffered operand images of a K chunk; then the ll tile or gamma [64][80]
ROWS = 64 * 8                          # the row of each frame of a tile
LSE = STAGE + ROWS + 2 * 64 * 4 * 8    # and the four online (max, sum) pairs per frame
GAMMA = STAGE + 2 * ROWS               # the rows and lse of the tile
STATS = STAGE + 32 * 80 * 8 + 2 * ROWS  # gamma over the staging, (1, x, x^2) of 32 frames, the rows and lse
TREE = 256 * 8                         # a block's fixed tree
BLOCK_LDS = 64 * 1024
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "gmm_offsets_kernel": ("gmm_offsets_kernel", TREE, 8),
    "gmm_prepare_kernel": ("gmm_prepare_kernel", 0, 8),
    "gmm_lse_kernelIfE": ("gmm_lse_kernel<float>", LSE, 3),
    "gmm_lse_kernelIdE": ("gmm_lse_kernel<double>", LSE, 3),
    "gmm_gamma_kernelIfE": ("gmm_gamma_kernel<float>", GAMMA, 3),
    "gmm_gamma_kernelIdE": ("gmm_gamma_kernel<double>", GAMMA, 3),
    "gmm_sums_kernel": ("gmm_sums_kernel", 2 * TREE, 8),
    "gmm_stats_kernelIfLb0E": ("gmm_stats_kernel<float, false>", STATS, 2),
    "gmm_stats_kernelIdLb0E": ("gmm_stats_kernel<double, false>", STATS, 2),
    "gmm_stats_kernelIfLb1E": ("gmm_stats_kernel<float, true>", STATS, 2),
    "gmm_stats_kernelIdLb1E": ("gmm_stats_kernel<double, true>", STATS, 2),
    "gmm_reduce_kernel": ("gmm_reduce_kernel", 0, 8),
    "gmm_mstep_weights_kernel": ("gmm_mstep_weights_kernel", TREE, 8),
    "gmm_mstep_moments_kernel": ("gmm_mstep_moments_kernel", 0, 8),
    "gmm_em_init_kernel": ("gmm_em_init_kernel", 0, 8),
    "gmm_em_check_kernel": ("gmm_em_check_kernel", 0, 8),
    "gmm_map_kernel": ("gmm_map_kernel", 0, 8),
    "gmm_super_model_kernel": ("gmm_super_model_kernel", 0, 8),
    "gmm_super_test_kernel": ("gmm_super_test_kernel", TREE, 8),
    "gmm_scores_kernel": ("gmm_scores_kernel", STAGE, 3),
}


@needs_hipcc
def test_gmm_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("gmm.hip")
    assert len(kernels) == len(KERNELS) == 20, sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*GMM-UBM", design, re.M).start():]
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
    # two blocks of the statistics kernel fit a CU's 160 KiB, three of the lse kernel
    assert 2 * STATS <= 160 * 1024 and 3 * LSE <= 160 * 1024
