"""Resource budget of the DER kernels (csrc/der.hip), compiled for gfx950 on the CPU: every kernel of the file is there, none
uses scratch or spills, and the LDS of each is what DESIGN.md ("DER") states: the pass's 64 x 64 histogram of 32-bit counts and
its four block sums; the solver's matrix as 32-bit values and the inverse map; a partial sum per thread where the rasteriser's
last block lays out the blocks of the pass; the two sums of the pooling block.  No kernel may use a float atomic."""
import os
import re

from conftest import ROOT
from hipcc_support import assert_no_scratch, header_constants, kernel_asm, kernel_instances, kernel_resources, needs_hipcc

C = header_constants("xvec_der.h", "XVEC_DER_")
CELLS = C["MAX_SPEAKERS"] ** 2
# kernel -> LDS bytes per block
KERNELS = {"der_raster_kernel": 4 * C["THREADS"], "der_pass_kernel": 4 * CELLS + 16, "der_assign_kernel": 4 * CELLS + 4 * C["MAX_SPEAKERS"],
           "der_pool_kernel": 16}


@needs_hipcc
def test_der_kernels_use_no_scratch_and_the_lds_the_design_states():
    kernels = kernel_resources("der.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want, lds in KERNELS.items():
        names = kernel_instances(kernels, want)
        assert len(names) == 1, (want, sorted(kernels))
        r = kernels[names[0]]
        assert_no_scratch(r, want, waves=1)
        assert r["lds"] == lds, (want, r)
        # DESIGN.md's table row: | `<kernel>` ... | <LDS bytes> |
        assert re.search(rf"\|\s*`{want}[^|\n]*\|\s*{lds:,}\s*\|", design), f"DESIGN.md does not state {lds:,} bytes of LDS for {want}"
    assert KERNELS["der_pass_kernel"] == 16400 and C["CHUNK_TICKS"] == C["THREADS"] * C["WAVE_ROWS"]
    # the pass fills a compute unit: eight waves a SIMD by registers, nine blocks by LDS
    assert kernels[kernel_instances(kernels, "der_pass_kernel")[0]]["occupancy"] == 8


@needs_hipcc
def test_der_kernels_use_integer_atomics_only():
    asm = kernel_asm("der.hip")
    atomics = set(re.findall(r"\b((?:global|flat|ds|buffer)_(?:atomic_)?(?:add|or|min|max|pk_add|cmpswap|cmpst)\w*)", asm))
    assert atomics, "no atomic found: the pattern no longer reads this compiler's assembly"
    assert not [a for a in atomics if re.search(r"f16|f32|f64|bf16", a)], atomics
    assert "cmpswap" not in " ".join(atomics) and "cmpst" not in " ".join(atomics), atomics      # no compare-and-swap loops either
