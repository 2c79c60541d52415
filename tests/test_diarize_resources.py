"""Resource budget of the clustering kernels (csrc/diar.hip), compiled for gfx950 on the CPU: every kernel of the file is there,
none uses scratch or spills, and the LDS of each is what DESIGN.md ("Diarization") states: per row of the recording the cached
best score and partner, the cluster size, the label and a place on the rescan list (24 bytes), the slots of the two block-wide
reductions (12 bytes per wave each) and the list's length, rounded up to 8 bytes."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

SMALL, LARGE, MAX_SEGMENTS = 64, 256, 2048          # tests/test_diarize.py ties the module's copies to the header
ROW_BYTES = 8 + 4 + 4 + 4 + 4
CLUSTER_LDS = lambda threads, rows: -(-(rows * ROW_BYTES + 2 * (threads // 64) * (8 + 4) + 4) // 8) * 8
# kernel -> LDS bytes per block of each instance
KERNELS = {
    "ahc_layout_kernel": [256 * 8],
    "ahc_init_kernel": [0],
    "ahc_cluster_kernel": [CLUSTER_LDS(SMALL, SMALL), CLUSTER_LDS(LARGE, MAX_SEGMENTS)],
}


@needs_hipcc
def test_diar_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("diar.hip")
    assert len(kernels) == sum(len(v) for v in KERNELS.values()), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, lds in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == len(lds), (want, sorted(kernels))
        for name in names:
            r = kernels[name]
            assert_no_scratch(r, name, waves=2)
        assert sorted(kernels[n]["lds"] for n in names) == sorted(lds), (want, [kernels[n] for n in names])
        for size in lds:
            if size:                            # DESIGN.md's table row: | `<kernel>` ... | <LDS bytes> |
                assert re.search(rf"\|\s*`{want}[^|\n]*\|\s*{size:,}\s*\|", design), \
                    f"DESIGN.md does not state {size:,} bytes of LDS for {want}"
    assert (CLUSTER_LDS(SMALL, SMALL), CLUSTER_LDS(LARGE, MAX_SEGMENTS)) == (1568, 49256)
    assert 3 * CLUSTER_LDS(LARGE, MAX_SEGMENTS) <= 160 * 1024          # three large blocks per CU
