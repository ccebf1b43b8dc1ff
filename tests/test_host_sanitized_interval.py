"""The host side of interval depth over many paths -- the batch plan, the windows of many paths and the BED name lookup of
flatgfa_core.cpp, which flatgfa_intervals_depth and the two tables on it run around the device's part -- under gcc's address
and undefined-behaviour sanitizers (CPU only), as tests/test_host_sanitized_topology.py does for validate and degree:
`make -C pollen_amd/csrc interval_host_check interval_host_asan` builds tests/host_check/interval_host_check.cpp twice; both
must finish clean and print the same, and the plain build's counts must be the model's."""
import glob
import os
import shutil
import subprocess

import pytest

import interval_model as im
from conftest import GOLDEN, ROOT
from oracle import flatgfa_oracle as fo

CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
BUILD = os.path.join(ROOT, "pollen_amd", "build")


@pytest.fixture(scope="module")
def binaries():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    subprocess.run(["make", "-C", CSRC, "interval_host_check", "interval_host_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "interval_host_check"), "asan": os.path.join(BUILD, "interval_host_check_asan")}


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.gfa")))


def parsable(path):
    try:
        return fo.parse_gfa(open(path, "rb").read())
    except fo.ParseError:
        return None


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe] + fixtures(), capture_output=True, text=True, timeout=600, env=env)


def test_interval_host_code_is_clean_and_agrees(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1].startswith("all ")
    by_file = {ln.split(" ")[0]: ln for ln in lines[:-1]}
    seen = 0
    for path in fixtures():
        p = parsable(path)
        if p is None or path not in by_file:
            continue
        seen += 1
        lens, _ = fo.path_depth(p)
        n_windows = sum(len(im.windows(int(n), w)) for n in lens for w in (1, 4, 2 ** 64 - 1))
        fields = dict(f.split("=") for f in by_file[path].split(" ")[1:])
        assert int(fields["windows"]) == n_windows, path
        # seams between two listed copies of one path: every path twice (one each that has windows) and thrice (two each); the
        # first path again behind all the others, as they are and with the others taken as windowless; at each of three sizes
        live = [int(n) > 0 for n in lens]
        seams = 3 * sum(live) + (int(live[0] and not any(live[1:])) + int(live[0]) if live else 0)
        assert int(fields["seams"]) == 3 * seams, path
        if len(p.paths):
            assert fields["refused"] == "1" and fields["refusals"] == "4", by_file[path]
    assert seen >= 5
    r = run(binaries["asan"])
    assert r.returncode == 0, f"asan: {r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"asan: {r.stderr[-3000:]}"
    assert r.stdout == plain.stdout
