"""Resource budget of the score-normalisation kernels (csrc/snorm.hip), compiled for gfx950 on the CPU: every kernel of the
file is there, none uses scratch or spills, and the LDS of each and the waves per SIMD it leaves are what DESIGN.md ("Score
normalisation") states: the key image of the row (8 bytes per cell) plus 1,128 bytes of histogram, scan and reduction words."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

SMALL, LARGE = 4096, 16384                     # XVEC_SNORM_RESIDENT_SMALL / _MAX (tests/test_snorm.py ties them to the header)
SIDE = 8 * 8 + 256 * 4 + 4 * 4 + 2 * 4 + 2 * 4 + 8       # wave sums, histogram, scan totals, chosen digit, two counters, the minimum
# kernel -> (LDS bytes per block, waves per SIMD: 512-thread blocks are two waves per SIMD each)
KERNELS = {
    "snorm_row_stats_kernelILi4096E": (8 * SMALL + SIDE, 8),
    "snorm_row_stats_kernelILi16384E": (8 * LARGE + SIDE, 2),
    "snorm_row_stats_kernelILi0E": (SIDE, 8),
    "snorm_apply_kernel": (0, 8),
}


@needs_hipcc
def test_snorm_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("snorm.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, (lds, occupancy) in KERNELS.items():
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] == lds and r["occupancy"] == occupancy, (want, r)
        blocks = 160 * 1024 // lds if lds else 8
        assert min(8, 2 * blocks) >= occupancy, (want, "the LDS image does not leave room for the blocks the occupancy counts")
        if lds:                                 # DESIGN.md's table row: | <cells> | <LDS bytes> | <blocks per CU> | <waves per SIMD> |
            row = re.search(rf"\|[^|\n]*\|\s*{lds:,}\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", design)
            assert row, f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
            assert int(row.group(1)) == min(4, blocks) and int(row.group(2)) == occupancy, (want, row.group(0))
    assert 160 * 1024 // (8 * SMALL + SIDE) == 4 and 160 * 1024 // (8 * LARGE + SIDE) == 1
