"""Resource budget of the augmentation kernels (csrc/augment.hip), compiled for gfx950 on the CPU: every kernel of the file is
there, none uses scratch or spills, and the LDS of every one fits a CU (160 KB); the convolution's (271 padded rows of x, 544
values of h, the reduction slots) leaves room for four blocks per CU.  Resource metadata only."""
from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

KERNELS = ("aug_mix_kernelILb0", "aug_mix_kernelILb1", "aug_reverb_conv_kernel", "aug_reverb_apply_kernel",
           "aug_normalize_kernel")
CONV_LDS = (271 * 33 + 544 + 4) * 4


@needs_hipcc
def test_augment_kernels_use_no_scratch():
    kernels = kernel_resources("augment.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] <= 160 * 1024, (want, r)
    conv = kernels[kernel_instances(kernels, "aug_reverb_conv_kernel")[0]]
    assert CONV_LDS <= conv["lds"] <= CONV_LDS + 16 and 4 * (CONV_LDS + 16) <= 160 * 1024, conv      # + alignment
    assert conv["occupancy"] >= 2, conv
