"""tools/print_cpu.cpp, the single-thread C++ restatement that tools/print_bench.py times, held against the host printer and
tests/print_model.py: on every golden graph, on the handmade texts and on pools that no text gives, and where the reference
panics it stops.  No GPU."""
import importlib.util
import os
import shutil

import pytest

import pollen_amd as pa
import print_model as pm
import print_shapes as ps
from conftest import ROOT, fixture_id, golden_gfas
from test_print_model import ERRORS, load


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    spec = importlib.util.spec_from_file_location("print_bench", os.path.join(ROOT, "tools", "print_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.build_cpu(str(tmp_path_factory.mktemp("print_cpu")))


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_golden(bench, gfa):
    mod, cpu = bench
    with open(gfa, "rb") as f, pa.parse_bytes(f.read()) as g:
        got = mod.run_cpu(cpu, g, True)
        assert got["text"] == g.gfa_text() == pm.gfa(pm.pools_of(g)) and got["bytes"] == len(got["text"])


def test_shapes(bench, tmp_path):
    mod, cpu = bench
    mod.restatement_is_the_printer(cpu)
    text = ps.alternating(12)
    for p in (ps.short_line_order(text, 7), ps.normalized(text), ps.shared_steps(text), ps.wide_ops(ps.long_cigar(30, 10))):
        with load(p, tmp_path) as g:
            assert mod.run_cpu(cpu, g, True)["text"] == g.gfa_text()


@pytest.mark.parametrize("message", list(ERRORS))
def test_stops_where_the_reference_panics(bench, message, tmp_path):
    mod, cpu = bench
    with load(ERRORS[message](), tmp_path) as g:
        with pytest.raises(AssertionError, match="the restatement stopped"):
            mod.run_cpu(cpu, g)
