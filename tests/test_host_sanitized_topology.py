"""The host side of validate and degree -- the two table formatters of flatgfa_core.cpp that flatgfa_validate_table and
flatgfa_degree_table call -- under the sanitizers gcc has (CPU only), as tests/test_host_sanitized.py does for the rest of
the host code: `make -C pollen_amd/csrc topology_check topology_asan topology_tsan` builds tests/host_check/topology_check.cpp
three ways; all three must finish clean, print the same, and the plain build's tables must have the size of the model's."""
import glob
import os
import shutil
import subprocess

import pytest

import topology_model as tm
from conftest import GOLDEN, ROOT
from oracle import flatgfa_oracle as fo

CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
BUILD = os.path.join(ROOT, "pollen_amd", "build")


@pytest.fixture(scope="module")
def binaries():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    subprocess.run(["make", "-C", CSRC, "topology_check", "topology_asan", "topology_tsan"], check=True, capture_output=True, timeout=600)
    return {k: os.path.join(BUILD, n) for k, n in (("plain", "topology_check"), ("asan", "topology_check_asan"), ("tsan", "topology_check_tsan"))}


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.gfa")) + glob.glob(os.path.join(GOLDEN, "topology", "*.dropped.gfa")))


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([exe] + fixtures(), capture_output=True, text=True, timeout=600, env=env)


def test_topology_formatters_are_clean_and_agree(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1].startswith("all ") and len(lines) == len(fixtures()) + 1
    for path, ln in zip(fixtures(), lines):
        p = fo.parse_gfa(open(path, "rb").read())
        assert ln == "%s validate=%d degree=%d ok=1 empty=1 refused=3" % (path, len(tm.validate_text(p)), len(tm.degree_text(p)))
    for kind in ("asan", "tsan"):
        r = run(binaries[kind])
        assert r.returncode == 0, f"{kind}: {r.stderr[-3000:]}"
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"{kind}: {r.stderr[-3000:]}"
        assert r.stdout == plain.stdout, kind
