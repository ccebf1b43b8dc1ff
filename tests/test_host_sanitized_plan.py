"""The host stages of the bucketed depth plan -- pollen_amd/csrc/depth_plan_host.hpp: which kernel walks which path, the cut
and the two deals, the tag verdict, pass 2's five lists, the item facts, the packed layout -- without a GPU and under gcc's
address and undefined-behaviour sanitizers, as tests/test_host_sanitized_interval.py does for interval depth:
`make -C pollen_amd/csrc plan_check plan_check_asan` builds tests/host_check/plan_check.cpp twice (against HIP's vector
types, nothing of its runtime); the program asserts what the kernels rely on, and both builds must finish clean and print
the same."""
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
    subprocess.run(["make", "-C", CSRC, "plan_check", "plan_check_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "plan_check"), "asan": os.path.join(BUILD, "plan_check_asan")}


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)


def test_plan_host_stages_hold_and_are_clean(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    for stage in ("cut ok", "classes ok", "tags ok", "lists ok", "layout ok", "item facts ok"):
        assert any(ln.startswith(stage) for ln in lines), stage
    r = run(binaries["asan"])
    assert r.returncode == 0, f"asan: {r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"asan: {r.stderr[-3000:]}"
    assert r.stdout == plain.stdout
