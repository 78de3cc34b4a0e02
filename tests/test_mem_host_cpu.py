"""The ownership types of the host layer (openwakeword_amd/csrc/owwhip_mem.h) as a stand-alone host program under AddressSanitizer + UBSan.

tests/mem_check.cpp includes only that header and defines its link-time seam over malloc / free with a live-allocation count, a call
log and a switch that fails the next allocation.  It checks: nothing live after any scope; move construction and assignment empty the
source and release the destination's old block once; reserve() within the capacity makes no seam call and keeps the pointer; growth
frees once, then allocates exactly n; a failed alloc / reserve leaves the buffer empty, returns the error, and the next one succeeds;
0 elements behave as max(n, 1); reset() twice is harmless; PinnedBuf hands its flags on; a borrowed stream is never destroyed; a
struct of several owners in an array and in a std::vector releases everything exactly once through reallocation, erase and resize.

Built with ROCm's host clang++ (-fsanitize=address,undefined -fno-sanitize-recover=undefined; without the sanitizers where a GPU is
present, so that no sanitizer runs on a shared GPU machine) and run as a process of its own -- it is never loaded into Python.
"""
import os
import re
import subprocess

import pytest

from test_pack_host_cpu import ROOT, _host_clangxx


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = _host_clangxx()
    if cxx is None:
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    exe = str(tmp_path_factory.mktemp("mem_check") / "mem_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "mem_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_every_check_passes_and_the_sanitizers_stay_silent(run):
    assert run.returncode == 0 and run.stderr == "", f"mem_check exit {run.returncode}:\n{run.stdout[-4000:]}\n{run.stderr[-4000:]}"
    m = re.fullmatch(r"ok (\d+) checks\n", run.stdout)
    assert m and int(m.group(1)) >= 60, run.stdout[-4000:]


def test_the_header_makes_no_hip_call_and_includes_no_hip_header():
    with open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip_mem.h")) as f:
        src = f.read()
    assert "#include <hip" not in src and not re.search(r"\bhip[A-Z]\w*\(", src)
