"""Resource budget of the VAD and CMVN kernels (csrc/vad.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills, and the LDS of each is what DESIGN.md ("Voice activity detection and sliding CMVN") states.
The normalise-and-select kernel's staged rows are dynamic LDS sized by the plan (csrc/vad_plan.h, at most XVEC_CMVN_LDS_BYTES);
its static part -- a frame's output row per frame of the tallest tile, the chunk's mask as a word per wave -- sits beside
them, and both together stay within the 64 KiB a block may ask for without an attribute, two blocks a CU."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

LANES, TILE_MAX, LDS_BYTES = 256, 256, 61440          # tests/test_vad.py ties the module's copies to the header
WAVES = LANES // 64
# kernel -> static LDS bytes per block
KERNELS = {
    "vad_decide_kernel": LANES * 8 + WAVES * 4,       # the partial sums, the waves' counts
    "vad_count_kernel": WAVES * 4,
    "cmvn_select_kernel": TILE_MAX * 4 + WAVES * 8,   # the output rows, the chunk's mask
}


@needs_hipcc
def test_vad_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("vad.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, lds in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == 1, (want, sorted(kernels))
        r = kernels[names[0]]
        assert_no_scratch(r, want, waves=4)
        assert r["lds"] == lds, (want, r)
        assert re.search(rf"\|\s*`{want}`[^|\n]*\|\s*{lds:,}\s*\|", design), f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
    total = KERNELS["cmvn_select_kernel"] + LDS_BYTES
    assert total <= 64 * 1024 and 2 * total <= 160 * 1024
