"""The lists the test support modules keep are the product's own: the dispatch knobs tdnn_support.make_model clears are the
ones xvec_create reads, and the flags hipcc_support compiles with are the ones the build compiles with.  Likewise the ids of
the segment layers' kernel forms: the C header, the host-only planner and the ctypes binding keep one list."""
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


def test_affine_form_ids_are_one_list():
    from xvector_amd import hip
    root = os.path.dirname(os.path.dirname(hipcc_support.CSRC))
    header = dict(re.findall(r"\bXVEC_AFFINE_(\w+) = (\d+)", open(os.path.join(root, "include", "xvec_hip.h")).read()))
    assert len(header) == 7
    names = {int(v): None if k == "NONE" else k.lower() for k, v in header.items()}
    assert names == hip.AFFINE_FORM_NAMES
    plan = re.search(r"enum Form \{(.*?)\};", open(os.path.join(hipcc_support.CSRC, "affine_plan.h")).read(), re.S).group(1)
    plan = re.sub(r"//[^\n]*", "", plan)
    ids = {k: int(v) for k, v in re.findall(r"\bk(\w+) = (\d+)", plan)}
    camel = {"None": "NONE", "Tile16": "TILE16", "Tile16Elem": "TILE16_ELEMENTWISE", "SplitK": "SPLITK", "SplitKX3": "SPLITK_BF16X3",
             "Direct": "DIRECT", "DirectX3": "DIRECT_BF16X3"}
    assert {camel[k]: v for k, v in ids.items()} == {k: int(v) for k, v in header.items()}
