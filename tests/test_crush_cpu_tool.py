"""tools/crush_cpu.cpp, the single-thread C++ restatement that tools/crush_bench.py times, held against tests/crush_model.py: on
every crush golden, on the shapes of tests/crush_shapes.py and on seeded random pools it writes the model's sequence pool and
prints the model's kept and dropped bytes and the checksum of the model's new lengths.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crush_model as cm
import crush_shapes as cs
import pollen_amd as pa
from conftest import ROOT
from test_crush_model import FIXTURES, random_pools


def checksum(a):
    a = np.asarray(a)
    return int(np.bitwise_xor.reduce(a.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.arange(len(a), dtype=np.uint64))) if len(a) else 0


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("crush_cpu") / "crush_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tools", "crush_cpu.cpp"), "-o", out], check=True)
    return out


def run_tool(tool, d, p):
    spans, pool, out = (str(d / n) for n in ("spans.bin", "pool.bin", "out.bin"))
    cm.seg_seq(p).tofile(spans)
    np.ascontiguousarray(p.seq_data).tofile(pool)
    return subprocess.run([tool, spans, pool, out], capture_output=True, timeout=120), out


def run_and_compare(tool, d, p, what=""):
    r, out = run_tool(tool, d, p)
    assert r.returncode == 0, r.stderr
    want = cm.crush_fast(p)
    lens = want.segs["seq_end"].astype(np.int64) - want.segs["seq_start"]
    assert [int(x) for x in r.stdout.split()[:3]] == [len(want.seq_data), cm.dropped(p), checksum(lens)], what
    with open(out, "rb") as f:
        assert f.read() == want.seq_data.tobytes(), what


def test_goldens(tool, tmp_path):
    for path in FIXTURES:
        g = pa.parse(path)
        run_and_compare(tool, tmp_path, cm.pools_of(g), path)
        g.close()


@pytest.mark.parametrize("name", [n for n in cs.SHAPES if n != "more tiles than workgroups"])
def test_shapes(tool, tmp_path, name):
    run_and_compare(tool, tmp_path, cs.SHAPES[name](), name)


def test_random_pools(tool, tmp_path):
    for seed in range(60):
        run_and_compare(tool, tmp_path, random_pools(seed), seed)


def test_a_span_outside_the_pool(tool, tmp_path):
    r, _ = run_tool(tool, tmp_path, cs.pools(b"ACGT", [(0, 4), (2, 5)]))
    assert r.returncode == 3 and b"segment 1" in r.stderr
