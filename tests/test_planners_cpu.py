"""The host planners without a GPU: csrc/owwhip_masked_host.h (group lists of a masked step), owwhip_bank_host.h (the bank's routing
table and refusals), owwhip_verifier_host.h (the per-stream verifier list, assignment checks) and owwhip_state_host.h (record layout,
group-block lists, refusals) as a plain host program (tests/planners_check.cpp) under AddressSanitizer / UBSan.  The program holds the
cases and their expectations; this file builds it once per test run, runs it as a process of its own and reads its "name value"
lines.  The three Python mirrors are held to the same program where they live: test_head_windows_cpu.py (bank_waves),
test_verifier_budget_cpu.py (sv_list) and test_range_guard_cpu.py (the record's two ends)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from openwakeword_amd import _build

from test_abi_cpu import ROOT
from test_pack_host_cpu import _host_clangxx

HEADERS = ("owwhip_masked_host.h", "owwhip_bank_host.h", "owwhip_verifier_host.h", "owwhip_state_host.h")


@functools.lru_cache(maxsize=None)
def planners_exe():
    """Path of the built check program (one build per test run, shared by the files that use it)."""
    cxx = _host_clangxx()
    if cxx is None or not os.path.exists(cxx):
        pytest.skip("ROCm's host clang++ (lib/llvm/bin/clang++ next to hipcc) is not installed")
    import torch
    d = tempfile.mkdtemp(prefix="planners_check")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "planners_check")
    sanitize = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, os.path.join(ROOT, "tests", "planners_check.cpp"),
                    "-I" + os.path.join(ROOT, "openwakeword_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe


def run_planners(*args):
    """stdout lines of one run; the run must end clean and silent."""
    env = {k: v for k, v in os.environ.items() if k != "OWW_BANK_WG"}
    run = subprocess.run([planners_exe(), *args], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", f"exit {run.returncode}:\n{run.stderr[-4000:]}"
    return run.stdout.splitlines()


@functools.lru_cache(maxsize=None)
def self_checks():
    """{name: value} of the program's own run: masked lists, bank route, assignment checks, state lists / refusals / layout."""
    return dict(ln.split(" ", 1) for ln in run_planners() if not ln.startswith("off"))


@functools.lru_cache(maxsize=None)
def record_offsets(has_vad):
    """{section: (first word, words)} of the default register-resident record as ows::layout places it."""
    out = {}
    for ln in run_planners():
        if ln.startswith("off%d " % int(has_vad)):
            _, name, first, words = ln.split()
            out[name] = (int(first), int(words))
    return out


def test_headers_are_free_of_hip_and_listed_as_build_inputs():
    deps = [os.path.basename(d) for d in _build.DEPS]
    with open(os.path.join(ROOT, "openwakeword_amd", "csrc", "owwhip.hip")) as f:
        lib = f.read()
    with open(os.path.join(ROOT, "tests", "planners_check.cpp")) as f:
        check = f.read()
    for name in HEADERS:
        with open(os.path.join(ROOT, "openwakeword_amd", "csrc", name)) as f:
            src = f.read()
        assert "#pragma once" in src and "hip/" not in src and "__global__" not in src and "__device__" not in src, name
        assert name in deps and f'#include "{name}"' in lib and f'#include "{name}"' in check, name
    # what moved is gone from the library's own file
    for gone in ("bank_quiesce", "int state_check_ids", "int state_check_headers", "void state_list_build", "bank_ntiles", "bank_wbytes"):
        assert gone not in lib, gone


def test_planners_under_the_sanitizers():
    got = self_checks()
    assert got["done"] == "1"
    # 12 sizes x (8 named masks + 3 random ones); 400 random subscription tables; 300 random id lists
    assert int(got["masked_cases"]) == 12 * 11 and int(got["bank_tables"]) == 400 and int(got["state_lists"]) == 300
    assert got["record_bytes0"] == "49344" and got["record_bytes1"] == str(49344 + 4 * (4 + 256))
