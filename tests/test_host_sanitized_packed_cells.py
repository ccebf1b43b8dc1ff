"""The packed cells of the sweep over the sorted record image -- pollen_amd/csrc/depth_sorted_host.hpp: a cell that holds the depth
difference in its low half and the revisit difference in its high half, the rule under which the halves never run into each
other, the packed sweep per record that k_accum_sorted runs -- without a GPU and under gcc's address and undefined-behaviour
sanitizers: `make -C pollen_amd/csrc packed_cells_check packed_cells_check_asan` builds tests/host_check/packed_cells_check.cpp
twice, a stand-alone program each; both must finish clean and print the same."""
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
    subprocess.run(["make", "-C", CSRC, "packed_cells_check", "packed_cells_check_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "packed_cells_check"), "asan": os.path.join(BUILD, "packed_cells_check_asan")}


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_packed_cells_match_brute_force_and_are_clean(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    for stage in ("round trip ok", "rule ok", "sweep ok", "bound ok"):
        assert any(ln.startswith(stage) for ln in lines), stage
    r = run(binaries["asan"])
    assert r.returncode == 0, f"asan: {r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"asan: {r.stderr[-3000:]}"
    assert r.stdout == plain.stdout
