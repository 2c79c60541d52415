"""What the CPU checks of the compiled kernels and of the host-only headers share: one hipcc command line (the build's own
code-generation flags, device code only), what it reports per kernel and the two assertions every resource test makes on that;
the dump programs of tests/abi/ built with the host compiler; the integer constants of a public header.  A plain module like
plda_em_ref.py; the test files import it."""
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


def kernel_instances(kernels, name):
    """The mangled names among `kernels` that are kernel `name`: its length-prefixed name with no further identifier character
    behind it, so the plain kernel and every instantiation of a template.  `name` may run on into the mangled template arguments
    ("aug_mix_kernelILb0") to pick single instantiations."""
    return [k for k in kernels if re.search(rf"\d{name}(?![a-z0-9_])", k)]


def assert_no_scratch(r, what, waves=0):
    """One kernel's report `r`: no scratch, no spilled register, at least `waves` waves per SIMD."""
    assert r["scratch"] == 0 and r.get("spill", 0) == 0, (what, r)
    assert r["occupancy"] >= waves, (what, r)


def header_constants(header, prefix):
    """{NAME: value} of the `#define <prefix>NAME <integer>` lines of include/`header`."""
    text = open(os.path.join(ROOT, "include", header)).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"#define {prefix}(\w+) (\d+)", text)}


def host_program(name, out_dir, *flags, include=()):
    """tests/abi/`name`.cpp (a stand-alone program over a host-only header of csrc/, or of the directories `include`) compiled
    with the host compiler into `out_dir`; returns ask(request lines) -> the program's answer lines, one per request.  For a
    program that answers otherwise, ask.output(*argv, stdin=None, text=True) is the whole standard output of one run."""
    exe = os.path.join(str(out_dir), name)
    src = os.path.join(ROOT, "tests", "abi", name + ".cpp")
    dirs = [arg for d in (CSRC, *include) for arg in ("-I", d)]
    out = subprocess.run([HOST_CXX, "-std=c++17", "-O1", "-Wall", *flags, *dirs, src, "-o", exe], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]

    def output(*argv, stdin=None, text=True):
        res = subprocess.run([exe, *argv], input=stdin, capture_output=True, text=text, timeout=300)
        assert res.returncode == 0, res.stderr[-500:]
        return res.stdout

    def ask(requests):
        lines = output(stdin="\n".join(requests) + "\n").splitlines()
        assert len(lines) == len(requests)
        return lines
    ask.output = output
    return ask
