"""Resource budget of the embedding-conditioning kernels (csrc/lda.hip with the statistics kernels of csrc/class_scatter.h it
instantiates), compiled for gfx950 on the CPU: every kernel of the file is there, none uses scratch or spills, and the LDS of each and the waves per SIMD it leaves are what DESIGN.md ("Embedding
conditioning") states: two double-buffered 16 x 80 images for the scatter, a 64 x 18 and a 16 x 80 image for the transform."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

SCATTER_LDS = 2 * 2 * 16 * 80 * 8               # sA, sB: two buffers of 16 rows x 80 doubles each
EMBED_LDS = 2 * 64 * 18 * 8 + 2 * 16 * 80 * 8   # sX: two buffers of 64 rows x 18 doubles; sW: two of 16 x 80
# kernel -> (instances, LDS bytes per block, waves per SIMD)
KERNELS = {
    "lda_class_sum_kernel": (2, 0, 8),
    "stats_mean_kernel": (1, 16 * 16 * 8, 8),
    "lda_class_mean_kernel": (1, 0, 8),
    "class_scatter_kernel": (4, SCATTER_LDS, 4),
    "class_scatter_reduce_kernel": (1, 0, 8),
    "embed_transform_kernel": (4, EMBED_LDS, 4),
    "embed_centre_kernel": (2, 0, 8),
}


@needs_hipcc
def test_lda_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("lda.hip")
    assert len(kernels) == sum(k[0] for k in KERNELS.values()), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, (count, lds, occupancy) in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == count, (want, sorted(kernels))
        for name in names:
            r = kernels[name]
            assert_no_scratch(r, name)
            assert r["lds"] == lds and r["occupancy"] == occupancy, (name, r)
        if lds > 4096:                          # DESIGN.md's table row: | <kernel> | <LDS bytes> | <blocks per CU> | <waves per SIMD> |
            assert 160 * 1024 // lds >= occupancy, (want, "the LDS image does not leave room for the blocks the occupancy counts")
            row = re.search(rf"\|\s*`{want}`\s*\|\s*{lds:,}\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", design)
            assert row, f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
            assert int(row.group(1)) == min(4, 160 * 1024 // lds) and int(row.group(2)) == occupancy, (want, row.group(0))
    assert (SCATTER_LDS, EMBED_LDS) == (40960, 38912)
