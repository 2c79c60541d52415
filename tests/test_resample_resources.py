"""Resource budget of the resampling kernels (csrc/resample.hip), compiled for gfx950 on the CPU: one kernel per input dtype and
accumulate mode, none uses scratch or spills, and each holds exactly the staged input span in LDS (XVEC_RESAMPLE_SPAN_MAX fp32
samples = 32 KiB), which leaves the five blocks per CU (five waves per SIMD) that DESIGN.md ("Resampling") states."""
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

SPAN_MAX = 8192                                # XVEC_RESAMPLE_SPAN_MAX (tests/test_resample.py ties it to the header)
KERNELS = ["resample_kernelIsLb1E", "resample_kernelIsLb0E", "resample_kernelIfLb1E", "resample_kernelIfLb0E"]


@needs_hipcc
def test_resample_kernels_use_no_scratch_and_stay_inside_the_lds_budget():
    kernels = kernel_resources("resample.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] == 4 * SPAN_MAX, (want, r)
        blocks = 160 * 1024 // r["lds"]                                   # 256-thread blocks: one wave per SIMD each
        assert blocks == 5 and r["occupancy"] == 5, (want, r)
        assert r["vgprs"] + r.get("agprs", 0) <= 512 // 5, (want, r)      # the registers leave room for those five waves
