"""Resource budget of the VBx kernels (csrc/vbx.hip), compiled for gfx950 on the CPU: every kernel of the file is there, none
uses scratch or spills, and the LDS of each is what DESIGN.md ("VBx") states: sqrt(phi) for the most dimensions, per speaker
the prior and the two constants of its model (24 bytes) and the first frame and new number of its label (8 bytes), a slot per
thread for the block-wide sum, and the 256 bytes the compiler keeps for the block-wide vote on the inputs."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, header_constants, kernel_instances, kernel_resources, needs_hipcc

C = header_constants("xvec_vbx.h", "XVEC_VBX_")
RUN_LDS = 8 * C["MAX_DIM"] + (3 * 8 + 2 * 4) * C["MAX_SPEAKERS"] + 8 * C["THREADS"] + 256
# kernel -> LDS bytes per block
KERNELS = {"vbx_init_kernel": 0, "vbx_run_kernel": RUN_LDS}


@needs_hipcc
def test_vbx_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("vbx.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, lds in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == 1, (want, sorted(kernels))
        r = kernels[names[0]]
        assert_no_scratch(r, want, waves=1)
        assert r["lds"] == lds, (want, r)
        if lds:                                 # DESIGN.md's table row: | `<kernel>` ... | <LDS bytes> |
            assert re.search(rf"\|\s*`{want}[^|\n]*\|\s*{lds:,}\s*\|", design), f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
    assert RUN_LDS == 8448
    # a block is four waves: whatever registers the recurrences' look-ahead takes, a compute unit holds a block or more
    assert kernels[kernel_instances(kernels, "vbx_run_kernel")[0]]["occupancy"] * 4 >= C["THREADS"] // 64
