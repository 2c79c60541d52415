"""Resource budget of the identification kernels (csrc/ident.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills (the 32-row slice and the sorted lists of up to 16 places stay in registers), and the LDS of
each is what DESIGN.md ("Speaker identification") states: three waves' partials of 64 columns, 20 bytes each for the column
statistics and 12 bytes per place of the list for the top-k walk."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

WAVES, COLS = 4, 64                            # XVEC_IDENT_COLS (tests/test_ident.py ties the module's copy to the header)
STATS_LDS = (WAVES - 1) * COLS * (8 + 8 + 4)   # m1, R, i1 of the waves 1 .. 3
LIST_LDS = lambda places: (WAVES - 1) * places * COLS * (8 + 4)
# kernel -> (instances, LDS bytes per block of each instance)
KERNELS = {
    "model_mean_kernel": (2, [0, 0]),
    "ident_col_stats_kernel": (1, [STATS_LDS]),
    "ident_col_merge_kernel": (1, [0]),
    "ident_open_set_kernel": (1, [0]),
    "ident_topk_kernel": (3, [LIST_LDS(1), LIST_LDS(4), LIST_LDS(16)]),
    "ident_topk_merge_kernel": (3, [0, 0, 0]),
}


@needs_hipcc
def test_ident_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("ident.hip")
    assert len(kernels) == sum(k[0] for k in KERNELS.values()), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, (count, lds) in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == count, (want, sorted(kernels))
        for name in names:
            r = kernels[name]
            assert_no_scratch(r, name, waves=2)
        assert sorted(kernels[n]["lds"] for n in names) == sorted(lds), (want, [kernels[n] for n in names])
        for size in lds:
            if size:                            # DESIGN.md's table row: | `<kernel>` ... | <LDS bytes> |
                assert re.search(rf"\|\s*`{want}[^|\n]*\|\s*{size:,}\s*\|", design), \
                    f"DESIGN.md does not state {size:,} bytes of LDS for {want}"
    assert (STATS_LDS, LIST_LDS(1), LIST_LDS(4), LIST_LDS(16)) == (3840, 2304, 9216, 36864)
