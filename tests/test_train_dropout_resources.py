"""Resource budget of the dropout instantiation of the training kernels (csrc/tdnn_train_dropout.hip), compiled for gfx950 on the
CPU: the file holds the two new kernels in both row forms -- the forward product with the mask in its epilogue
(train_gemm_kernel<OP_FWD_DROPOUT = 3, ...>) and the dz kernel that carries the scale -- next to its own copies of the kernels the
calls share with the ones without dropout, and nothing else; none uses scratch or spills; the product kernels keep the LDS of
tests/test_train_resources.py (the Philox rounds of the epilogue live in registers) and at least two waves per SIMD.  The files
without dropout must not have gained a kernel: tests/test_train_resources.py and tests/test_train_ragged.py count theirs.
Resource metadata only."""
import shutil
import subprocess

import pytest

from hipcc_support import assert_no_scratch, kernel_instances, kernel_resources, needs_hipcc

GEMM_LDS = 2 * 2 * 16 * 132 * 4
# OP 3: forward with dropout; OP 1, 2: the dW and dx products, unchanged by dropout.  (vec, ragged) in every combination.
DROPOUT_GEMMS = tuple(f"train_gemm_kernelILi3ELb{vec}ELb{ragged}E" for vec in (0, 1) for ragged in (0, 1))
SHARED_GEMMS = tuple(f"train_gemm_kernelILi{op}ELb{vec}ELb{ragged}E" for op in (1, 2) for vec in (0, 1) for ragged in (0, 1))
DROPOUT_DZ = tuple(f"train_dz_dropout_kernelILb{ragged}E" for ragged in (0, 1))
SHARED = tuple(f"{name}ILb{ragged}E" for name in ("train_stats_kernel", "train_stats_merge_kernel", "train_norm_kernel",
                                                   "train_bn_sums_kernel") for ragged in (0, 1)) + (
    "train_slab_reduce_kernel", "train_col_reduce_kernel")
KERNELS = DROPOUT_GEMMS + SHARED_GEMMS + DROPOUT_DZ + SHARED


@needs_hipcc
def test_dropout_kernels_use_no_scratch():
    kernels = kernel_resources("tdnn_train_dropout.hip")
    assert len(kernels) == len(KERNELS) == 24, sorted(kernels)
    for want in KERNELS:
        name = kernel_instances(kernels, want)
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert_no_scratch(r, want)
        assert r["lds"] <= 160 * 1024, (want, r)
    for want in DROPOUT_GEMMS + SHARED_GEMMS:
        r = kernels[kernel_instances(kernels, want)[0]]
        assert r["lds"] == GEMM_LDS and 4 * GEMM_LDS <= 160 * 1024, (want, r)
        assert_no_scratch(r, want, waves=2)


@needs_hipcc
def test_dropout_lives_in_its_own_file_only():
    """No forward product without dropout, and no plain dz kernel, is compiled into the dropout file; no dropout kernel into the
    other two."""
    mine = kernel_resources("tdnn_train_dropout.hip")
    assert not [k for k in mine if "train_gemm_kernelILi0E" in k or "train_dz_kernel" in k]
    for src in ("tdnn_train.hip", "tdnn_train_ragged.hip"):
        assert not [k for k in kernel_resources(src) if "train_gemm_kernelILi3E" in k or "dropout" in k.split("GemmArgs")[0]], src


@needs_hipcc
@pytest.mark.skipif(shutil.which("nm") is None, reason="needs binutils nm")
@pytest.mark.parametrize("src", ["tdnn_train.hip", "tdnn_train_ragged.hip", "tdnn_train_dropout.hip"])
def test_host_and_device_agree_on_the_kernel_names(src):
    """The kernels' parameter list depends on OP (the trailing Dropout<OP == OP_FWD_DROPOUT>), so that expression is part of
    their mangled names: every kernel of the device code must be a symbol of the built library under exactly that name -- the
    runtime looks a kernel up by the host's spelling, and a launch of one it cannot find aborts the process.  (An unnamed
    enumeration in that expression is numbered differently by the host and the device compilation.)"""
    from xvector_amd import hip
    host = set(subprocess.run(["nm", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout.split())
    missing = [k for k in kernel_resources(src) if k not in host]
    assert not missing, missing
