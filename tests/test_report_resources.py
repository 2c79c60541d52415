"""Resource budget of the trial-report kernels (csrc/report.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills, and the LDS of each and the waves per SIMD it leaves are what DESIGN.md ("Trial report")
states in its table, row by row."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

SCAN = 4 * 4                   # the wave totals of a block scan: four words
WORDS = 4 * 8                  # the waves' partial results of a block reduction: four doubles (or int64)
TILE = 4096                    # XVEC_REPORT_TILE staged cells: a value (1 or 4 bytes) and a flag byte each
# kernel (mangled template arguments where there are instantiations) -> (its name in DESIGN.md, LDS bytes per block, waves per SIMD)
KERNELS = {
    "report_map_kernel": ("report_map_kernel", 4, 8),
    "report_range_kernel": ("report_range_kernel", 2 * WORDS, 8),
    "report_range_final_kernel": ("report_range_final_kernel", 2 * WORDS, 8),
    "report_images_kernelIhE": ("report_images_kernel<uint8_t>", TILE * 2, 8),
    "report_images_kernelIfE": ("report_images_kernel<float>", TILE * 5, 8),
    "report_det_prepare_kernelILb0E": ("report_det_prepare_kernel<false>", 8, 8),
    "report_det_prepare_kernelILb1E": ("report_det_prepare_kernel<true>", 8, 8),
    "report_det_sums_kernel": ("report_det_sums_kernel", SCAN, 8),
    "report_det_scan_kernel": ("report_det_scan_kernel", SCAN, 8),
    "report_det_points_kernelILb0E": ("report_det_points_kernel<false>", SCAN, 8),
    "report_det_points_kernelILb1E": ("report_det_points_kernel<true>", SCAN, 8),
    "report_det_keep_kernel": ("report_det_keep_kernel", SCAN, 8),
    "report_det_keep_scan_kernel": ("report_det_keep_scan_kernel", SCAN, 8),
    "report_det_compact_kernel": ("report_det_compact_kernel", SCAN, 8),
    "report_det_header_kernel": ("report_det_header_kernel", 0, 8),
}


@needs_hipcc
def test_report_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("report.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[re.search(r"^## [^\n]*Trial report", design, re.M).start():]
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
    assert 160 * 1024 // (TILE * 5) >= 8          # the float tile leaves room for the eight blocks of four waves a CU's wave slots hold
