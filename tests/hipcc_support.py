"""What the CPU checks of the compiled kernels share: one hipcc command line (the build's own code-generation flags, device
code only) and what it reports per kernel.  A plain module like plda_em_ref.py; the test files import it."""
import functools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "speaker-recognition-x-vectors_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
needs_hipcc_and_make = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="needs hipcc")
# csrc/Makefile's CXXFLAGS without the host half (tests/test_support_modules.py ties the two)
DEVICE_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-fno-slp-vectorize", "-Wno-unused-function",
                "-Wno-pass-failed", "-Wno-inline-asm"]
HOST_CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
needs_host_cxx = pytest.mark.skipif(HOST_CXX is None, reason="needs a C++ compiler")
_REPORT = (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
           ("agprs", r" AGPRs: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def _hipcc(*args):
    out = subprocess.run([HIPCC, *DEVICE_FLAGS, *args], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


@functools.lru_cache(maxsize=None)
def kernel_resources(src):
    """{mangled kernel name: {scratch, spill, vgprs, agprs, occupancy, lds}} of csrc/`src`, as hipcc's
    -Rpass-analysis=kernel-resource-usage reports them; compiled once per source and session."""
    kernels, name = {}, None
    for line in _hipcc("-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull).stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in _REPORT:
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    return kernels


def kernel_asm(src):
    """The gfx950 assembly of csrc/`src`."""
    return _hipcc("-S", src, "-o", "-").stdout


def host_program(name, out_dir, *flags):
    """tests/abi/`name`.cpp (a stand-alone program over a host-only header of csrc/) compiled with the host compiler into
    `out_dir`; returns ask(request lines) -> the program's answer lines, one per request."""
    exe = os.path.join(str(out_dir), name)
    src = os.path.join(ROOT, "tests", "abi", name + ".cpp")
    out = subprocess.run([HOST_CXX, "-std=c++17", "-O1", "-Wall", *flags, "-I", CSRC, src, "-o", exe], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]

    def ask(requests):
        res = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-500:]
        lines = res.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return ask
