"""The host's stages of flatgfa_flip -- pollen_amd/csrc/flip_host.hpp: how the paths are laid one behind another, what is
checked before anything is uploaded, the names of the turned paths, the assembly of the new store -- under the sanitizers gcc
has (CPU only), as tests/test_host_sanitized_topology.py does for validate's host side: `make -C pollen_amd/csrc
flip_host_check flip_host_asan` builds tests/host_check/flip_host_check.cpp (a program of its own, with its own main) twice;
both must finish clean and print the same, and the plain build's numbers must be the model's."""
import glob
import os
import shutil
import subprocess

import pytest

import flip_model as fm
import pollen_amd as pa
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
BUILD = os.path.join(ROOT, "pollen_amd", "build")


@pytest.fixture(scope="module")
def binaries():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    subprocess.run(["make", "-C", CSRC, "flip_host_check", "flip_host_asan"], check=True, capture_output=True, timeout=600)
    return {"plain": os.path.join(BUILD, "flip_host_check"), "asan": os.path.join(BUILD, "flip_host_check_asan")}


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))) + [os.path.join(GOLDEN, "flip", "synth_flip.gfa.txt")]


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe] + fixtures(), capture_output=True, text=True, timeout=600, env=env)


def test_flip_host_stages_are_clean_and_agree_with_the_model(binaries):
    plain = run(binaries["plain"])
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert lines[-1].startswith("all ") and lines[-1].endswith(" refused=10") and len(lines) == len(fixtures()) + 1
    for path, ln in zip(fixtures(), lines):
        g = pa.parse(path)
        q = fm.flip(fm.pools_of(g))
        n_turned = int(fm.turned(fm.pools_of(g)).sum())
        g.close()
        assert ln == "%s paths=%d turned=%d steps=%d links=%d names=%d alignment=%d again=1" % (
            path, len(q.paths), n_turned, len(q.steps), len(q.links), len(q.name_data), len(q.alignment))
    r = run(binaries["asan"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout == plain.stdout
