"""tools/bed_cpu.cpp, the single-thread C++ restatement that tools/bed_bench.py times (the device's method: grouping and
bisection), held against tests/bed_model.py (the reference's double loop): the text on every shape and on a seeded random
slice, and where the reference panics it stops.  No GPU."""
import importlib.util
import os
import random
import shutil

import pytest

import bed_model as bm
import bed_shapes as bs
from conftest import ROOT


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    spec = importlib.util.spec_from_file_location("bed_bench", os.path.join(ROOT, "tools", "bed_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.build_cpu(str(tmp_path_factory.mktemp("bed_cpu")))


@pytest.mark.parametrize("name", list(bs.SHAPES))
def test_shapes(bench, name):
    mod, cpu = bench
    a, b = bs.SHAPES[name]
    got = mod.run_cpu(cpu, a, b, True)
    want = bm.intersect(a, b)
    assert got["text"] == want and got["stats"][:2] == (want.count(b"\n"), len(want)) and got["stats"][2] >= got["stats"][0]


def test_counts_of_the_pruning(bench):
    mod, cpu = bench
    assert mod.run_cpu(cpu, *bs.SHAPES["nested b"])["stats"] == (1, 10, 3, 0)
    assert mod.run_cpu(cpu, *bs.SHAPES["equal starts"])["stats"][2:] == (3, 0)
    assert mod.run_cpu(cpu, *bs.SHAPES["unsorted group"])["stats"][3] == 1
    a, b = b"x\t0\t%d\n" % 5000, bs.text(bs.run(b"x", 500))
    assert mod.run_cpu(cpu, a, b)["stats"][::2] == (500, 500)


def test_random_slice(bench):
    mod, cpu = bench
    rng = random.Random(77)
    for _ in range(150):
        a, b = bs.random_case(rng)
        assert mod.run_cpu(cpu, a, b, True)["text"] == bm.intersect(a, b)


@pytest.mark.parametrize("bad", [b"x\n", b"x\t1\n", b"x\t1\tq\n"])
def test_stops_where_the_reference_panics(bench, bad):
    mod, cpu = bench
    with pytest.raises(bm.BedError):
        bm.parse(bad)
    for a, b in ((bad, b"x\t1\t2\n"), (b"x\t1\t2\n", bad)):
        with pytest.raises(AssertionError, match="the restatement stopped"):
            mod.run_cpu(cpu, a, b)


def test_the_bench_shapes(bench):
    """the synthetic texts at a small size: sorted, parseable, about two hits an A line; nested: every candidate range begins
    at its group's head"""
    mod, cpu = bench
    a = mod.synth(cpu, 400, 0, 10, 140)
    b = mod.synth(cpu, 40, 20, 100, 60)
    nested = mod.synth(cpu, 40, 20, 100, 60, 5000)
    assert a.count(b"\n") == 400 * mod.NAMES and b.count(b"\n") == 40 * mod.NAMES and nested.count(b"\n") == 41 * mod.NAMES
    assert a.startswith(b"chr1\t0\t140\nchr1\t10\t150\n") and nested.startswith(b"chr1\t0\t5000\nchr1\t20\t80\n")
    for text in (b, nested):
        got = mod.run_cpu(cpu, a, text, True)
        assert got["text"] == bm.intersect(a, text) and got["stats"][3] == 0
    plain, deep = mod.run_cpu(cpu, a, b)["stats"], mod.run_cpu(cpu, a, nested)["stats"]
    assert 1.5 < plain[0] / a.count(b"\n") < 2.5 and plain[2] == plain[0]
    assert deep[0] == plain[0] + a.count(b"\n") and deep[2] > 5 * deep[0]
