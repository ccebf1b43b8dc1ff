"""tools/flip_cpu.cpp, the single-thread C++ restatement that tools/flip_bench.py times, held against tests/flip_model.py: on
every flip golden's input and on the shapes of tests/flip_shapes.py it writes the model's steps, turned flags and links and
prints the model's counts.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flip_model as fm
import flip_shapes as fs
import pollen_amd as pa
from conftest import ROOT
from test_flip_model import FIXTURES

FILES = ("steps.bin", "spans.bin", "seglen.bin", "links.bin", "align.bin", "out_steps.bin", "out_turned.bin", "out_links.bin")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("flip_cpu") / "flip_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tools", "flip_cpu.cpp"), "-o", out], check=True)
    return out


def run_tool(tool, d, p):
    paths = [str(d / n) for n in FILES]
    spans = np.zeros(2 * len(p.paths), np.uint32)
    spans[0::2], spans[1::2] = p.paths["steps_start"], p.paths["steps_end"]
    arrays = (p.steps, spans, (p.segs["seq_end"] - p.segs["seq_start"]).astype(np.uint32), p.links, p.alignment.astype(np.uint32))
    for a, path in zip(arrays, paths):
        np.ascontiguousarray(a).tofile(path)
    return subprocess.run([tool] + paths, capture_output=True, timeout=120), paths[5:]


def run_and_compare(tool, d, p, what=""):
    r, outs = run_tool(tool, d, p)
    assert r.returncode == 0, r.stderr
    want, t = fm.flip(p), fm.turned(p)
    new = sum(1 for ln in want.links if int(ln["ov_start"]) == len(p.alignment) and int(ln["ov_end"]) == len(p.alignment) + 1)
    assert [int(x) for x in r.stdout.split()[:3]] == [int(t.sum()), len(want.links), new], what
    for path, a in zip(outs, (want.steps, t.astype(np.uint8), want.links)):
        with open(path, "rb") as f:
            assert f.read() == a.tobytes(), (what, path)


def test_goldens(tool, tmp_path):
    for path in FIXTURES:
        g = pa.parse(path)
        run_and_compare(tool, tmp_path, fm.pools_of(g), path)
        g.close()


@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_shapes(tool, tmp_path, name):
    run_and_compare(tool, tmp_path, fs.SHAPES[name](), name)


def test_what_is_out_of_range(tool, tmp_path):
    p = fs.graph([2, 2], [[0, 3]], [(0, 2, [0])])
    p.steps[1] = 4
    r, _ = run_tool(tool, tmp_path, p)
    assert r.returncode == 3 and b"a step names no segment" in r.stderr
    p = fs.graph([2, 2], [[0, 3]], [(0, 2, [0])])
    p.links[0] = (0, 2, 0, 2)
    r, _ = run_tool(tool, tmp_path, p)
    assert r.returncode == 3 and b"link 0" in r.stderr
