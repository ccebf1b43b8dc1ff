"""The host's decisions about one call of a bucketed depth plan -- pollen_amd/csrc/depth_call_host.hpp: the shape of the call
(which launches, how large, who zeroes what), the build of k_scan, and what a status word asks for -- without a GPU and under
gcc's address and undefined-behaviour sanitizers, as tests/test_host_sanitized_plan.py does for the plan's creation:
`make -C pollen_amd/csrc call_check call_check_asan` builds tests/host_check/call_check.cpp twice (against HIP's vector
types, nothing of its runtime); the program runs the functions over every combination of the facts they read and asserts
what the kernels and the handle rely on, and both builds must finish clean and print the same."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
BUILD = os.path.join(ROOT, "pollen_amd", "build")


@pytest.fixture(scope="module")
def binaries():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    subprocess.run(["make", "-C", CSRC, "call_check", "call_check_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "call_check"), "asan": os.path.join(BUILD, "call_check_asan")}


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)


def test_call_decisions_hold_and_are_clean(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    for part in ("shapes ok", "path sums ok", "status ok"):
        assert any(ln.startswith(part) for ln in lines), part
    r = run(binaries["asan"])
    assert r.returncode == 0, f"asan: {r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"asan: {r.stderr[-3000:]}"
    assert r.stdout == plain.stdout
