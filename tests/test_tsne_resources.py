"""Resource budget of the t-SNE kernels (csrc/tsne.hip), compiled for gfx950 on the CPU: every kernel of the file is there,
none uses scratch or spills a vector register, and the LDS of each is what DESIGN.md ("Embedding maps") states.  The pair pass
and the KL pass stage a slice's y as XVEC_TSNE_SLICE_MAX double2 -- half of the 64 KiB a block may ask for without an
attribute; the affinity kernel keeps a row's distances in registers, 8 or 32 a thread."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

WAVES, SLICE_MAX, TILE = 4, 2048, 32                  # tests/test_tsne.py ties the header's constants to the module
# kernel -> (instantiations, static LDS bytes per block, waves per SIMD at least)
KERNELS = {
    "tsne_widen_kernel": (2, 0, 8),                   # fp32 and fp64 input
    "tsne_sqdist_kernel": (1, 0, 8),
    "tsne_affinity_kernel": (2, 2 * WAVES * 2 * 8 + WAVES * 8, 2),      # 8 and 32 distances a thread
    "tsne_total_kernel": (1, WAVES * 8, 8),
    "tsne_symmetrize_kernel": (1, 2 * TILE * (TILE + 1) * 8, 8),
    "tsne_pair_kernel": (2, SLICE_MAX * 16, 4),       # 16-byte and 8-byte loads of P
    "tsne_update_kernel": (1, WAVES * 8, 8),
    "tsne_z_kernel": (1, WAVES * 8, 8),
    "tsne_kl_kernel": (2, SLICE_MAX * 16, 4),
    "tsne_finish_kernel": (1, WAVES * 8, 8),
}


@needs_hipcc
def test_tsne_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("tsne.hip")
    assert len(kernels) == sum(count for count, _, _ in KERNELS.values()), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, (count, lds, occupancy) in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == count, (want, sorted(kernels))
        for name in names:
            r = kernels[name]
            assert_no_scratch(r, name, waves=occupancy)
            assert r["lds"] == lds, (name, r)
        assert re.search(rf"\|\s*`{want}`[^|\n]*\|\s*{lds:,}\s*\|", design), f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
    assert KERNELS["tsne_pair_kernel"][1] <= 32 * 1024      # two blocks a CU beside each other with room to spare
