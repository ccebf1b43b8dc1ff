"""tools/inject_cpu.cpp, the single-thread C++ restatement that tools/inject_bench.py times, held against tests/inject_model.py:
on every inject golden and on seeded random graphs it gives the model's step, segment and path counts and the checksums of
the model's steps, segment lengths and path spans.  No GPU."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import inject_model as im
from conftest import GOLDEN, ROOT
from oracle import flatgfa_oracle as fo
from test_inject_model import random_case

HERE = os.path.join(GOLDEN, "inject")
FIXTURES = sorted(os.path.basename(p)[:-len(".inject.bed")] for p in glob.glob(os.path.join(HERE, "*.inject.bed")))


def checksum(a):
    a = np.asarray(a)
    return int(np.bitwise_xor.reduce(a.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.arange(len(a), dtype=np.uint64))) if len(a) else 0


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("inject_cpu") / "inject_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tools", "inject_cpu.cpp"), "-o", out], check=True)
    return out


def run_and_compare(tool, tmp_path, p, lines):
    flat, bed = str(tmp_path / "g.flatgfa"), str(tmp_path / "l.bed")
    with open(flat, "wb") as f:
        f.write(fo.dump_flatgfa(p))
    with open(bed, "wb") as f:
        f.write(b"# a comment\n\n" + im.bed_text(lines))
    r = subprocess.run([tool, flat, bed], check=True, capture_output=True, timeout=120)
    got = [int(x) for x in r.stdout.split()[:6]]
    want = im.inject(p, lines)
    lens = want.segs["seq_end"].astype(np.int64) - want.segs["seq_start"]
    spans = np.concatenate([want.paths["steps_start"], want.paths["steps_end"]])
    assert got == [len(want.steps), len(want.segs), len(want.paths), checksum(want.steps), checksum(lens), checksum(spans)]


@pytest.mark.parametrize("stem", FIXTURES)
def test_goldens(tool, tmp_path, stem):
    text = open(os.path.join(HERE if stem == "synth_inject" else GOLDEN, stem + ".gfa"), "rb").read()
    p = fo.parse_gfa(text if text.endswith(b"\n") else text + b"\n")
    bed = open(os.path.join(HERE, stem + ".inject.bed"), "rb").read()
    lines = [(f[0], int(f[1]), int(f[2]), f[3]) for f in (ln.split(b"\t") for ln in bed.splitlines())]
    run_and_compare(tool, tmp_path, p, lines)


def test_random_graphs(tool, tmp_path):
    rng = np.random.default_rng(5)
    for _ in range(40):
        p, lines = random_case(rng)
        run_and_compare(tool, tmp_path, p, lines)
