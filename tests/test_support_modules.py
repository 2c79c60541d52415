"""The lists the test support modules keep are the product's own: the dispatch knobs tdnn_support.make_model clears are the
ones xvec_create reads, and the flags hipcc_support compiles with are the ones the build compiles with."""
import os
import re

import hipcc_support
import tdnn_support

ANALYSIS_ONLY = ("--cuda-device-only", "-S", "-c", "-o")    # (and -Rpass-analysis=...) make a device-only analysis compile


def test_knobs_are_the_ones_read_policy_reads():
    src = open(os.path.join(hipcc_support.CSRC, "xvec_api.hip")).read()
    read = set(re.findall(r'env_int\("(XVEC_\w+)"', src))
    assert read == set(tdnn_support.KNOBS), f"in one list only: {sorted(read ^ set(tdnn_support.KNOBS))}"


def test_device_flags_are_the_build_s_code_generation_flags():
    make = open(os.path.join(hipcc_support.CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", make, re.M).group(1)
    cxxflags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", make, re.M).group(1).replace("$(ARCH)", arch).split()
    for flag in hipcc_support.DEVICE_FLAGS:
        assert flag in ANALYSIS_ONLY or flag.startswith("-Rpass-analysis=") or flag in cxxflags, \
            f"{flag} is not in the Makefile's CXXFLAGS"
    codegen = [f for f in cxxflags if f.startswith(("-O", "-std", "-f", "--offload-arch")) and f != "-fPIC"]
    assert len(codegen) >= 4, codegen
    for flag in codegen:
        assert flag in hipcc_support.DEVICE_FLAGS, f"CXXFLAGS' {flag} is missing from hipcc_support.DEVICE_FLAGS"
