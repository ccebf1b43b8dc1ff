"""The sweep over groups of four chunks of the sorted record image -- the per-lane arithmetic of pollen_amd/csrc/depth_sorted_host.hpp
that k_accum_sorted runs: a record's key from the ordinal the image carries, the chunk's seed, the step that finds a revisit --
on a host model of the finaliser's image against brute force, without a GPU and under gcc's address and undefined-behaviour
sanitizers, as tests/test_host_sanitized_sorted.py does for the image's layout: `make -C pollen_amd/csrc sorted_group_check
sorted_group_check_asan` builds tests/host_check/sorted_group_check.cpp twice; both builds must finish clean and print the same."""
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
    subprocess.run(["make", "-C", CSRC, "sorted_group_check", "sorted_group_check_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "sorted_group_check"), "asan": os.path.join(BUILD, "sorted_group_check_asan")}


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_the_group_sweep_matches_brute_force_and_is_clean(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    for stage in ("record word ok", "groups ok"):
        assert any(ln.startswith(stage) for ln in lines), stage
    r = run(binaries["asan"])
    assert r.returncode == 0, f"asan: {r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"asan: {r.stderr[-3000:]}"
    assert r.stdout == plain.stdout
