"""tests/topology_model.py against the reference's own output (tests/golden/topology/, written by slow_odgi validate, degree
and validate_setup: make_topology_golden.py), the rules one by one on hand-made pools, the planted shapes of
tests/topology_shapes.py against their hand-derived answers, and the new entry points in the built library.  No GPU."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import random_pools as rp
import topology_model as tm
import topology_shapes as ts
from conftest import GOLDEN, fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

TOPO = os.path.join(GOLDEN, "topology")
MANIFEST = json.load(open(os.path.join(TOPO, "MANIFEST.json")))


def golden(name: str) -> bytes:
    data = open(os.path.join(TOPO, name), "rb").read()
    assert hashlib.sha256(data).hexdigest() == MANIFEST[name]["sha256"], name
    return data


def read_gfa(path) -> bytes:
    """The fixture as mygfa reads it: ref_handmade_no-test-flip4.gfa ends without a newline, and the flatgfa parser (the
    oracle's and the library's alike) reads no line that is not terminated -- there its L line -- where mygfa reads it."""
    data = open(path, "rb").read()
    return data if data.endswith(b"\n") else data + b"\n"


def oracle_parses(path) -> bool:
    try:
        fo.parse_gfa(read_gfa(path))
        return True
    except fo.ParseError:
        return False


def test_every_golden_gfa_has_reference_output():
    for path in golden_gfas():
        for suffix in (".validate.txt", ".degree.tsv", ".dropped.gfa", ".dropped.validate.txt"):
            assert fixture_id(path) + suffix in MANIFEST
    assert [fixture_id(p) for p in golden_gfas() if not oracle_parses(p)] == []


@pytest.mark.parametrize("path", golden_gfas(), ids=fixture_id)
def test_model_equals_slow_odgi_on_goldens(path):
    name = fixture_id(path)
    p = fo.parse_gfa(read_gfa(path))
    assert tm.validate_text(p) == golden(name + ".validate.txt")
    assert tm.degree_text(p) == golden(name + ".degree.tsv")
    q = fo.parse_gfa(golden(name + ".dropped.gfa"))
    assert tm.validate_text(q) == golden(name + ".dropped.validate.txt")
    assert len(q.links) == int(0.1 * len(p.links))  # validate_setup.py:12


def test_both_outcomes_are_pinned():
    lines = {fixture_id(p): (MANIFEST[fixture_id(p) + ".validate.txt"]["lines"], MANIFEST[fixture_id(p) + ".dropped.validate.txt"]["lines"])
             for p in golden_gfas()}
    assert sum(1 for a, _ in lines.values() if a == 0) == 6 and all(b > 0 for _, b in lines.values())
    assert lines["ref_ex2"] == (0, 8) and lines["ref_handmade_crush1"] == (0, 17) and lines["ref_handmade_flip3"][1] == 9


def test_model_equals_slow_odgi_on_the_synthetic_graph():
    p = ts.synth_mid()
    assert hashlib.sha256(ts.gfa_text(p)).hexdigest() == MANIFEST["synth_mid.gfa"]["sha256"]  # the graph the reference was given
    assert 7000 < len(p.segs) < 9000 and 90_000 < len(p.steps) < 110_000
    text = tm.validate_text(p)
    assert text == golden("synth_mid.validate.txt") and text.count(b"\n") == 440
    assert tm.degree_text(p) == golden("synth_mid.degree.tsv")
    assert len(text) < os.path.getsize(os.path.join(GOLDEN, "synth_cfgS.depth.tsv"))


@pytest.mark.parametrize("seed", rp.TEXT_SEEDS)
def test_model_equals_slow_odgi_on_random_graphs(seed):
    """random_pools' text profile: dropped links, both spellings, duplicates, self-loops, x+ -> x-, a hub row, sparse names."""
    p = rp.make(seed, "text")
    assert hashlib.sha256(rp.gfa_text(p)).hexdigest() == MANIFEST["random_%d.gfa" % seed]["sha256"]  # the graph the reference was given
    text = tm.validate_text(p)
    assert text == golden("random_%d.validate.txt" % seed) and text.count(b"\n") > 10
    assert tm.degree_text(p) == golden("random_%d.degree.tsv" % seed)


# ---- the rules, one by one: handles are segment << 1 | backward; segments 0, 1, 2 are named 1, 2, 3 ----
A, B, C = 0, 2, 4


def recs(p):
    return [(int(r["path"]), int(r["step"]), int(r["src"]), int(r["dst"])) for r in tm.validate(p)]


def test_forward_and_reverse_form_support():
    assert recs(ts.make_pools(3, [A, B], [(0, 2)], [(A, B)])) == []
    assert recs(ts.make_pools(3, [A, B], [(0, 2)], [(B ^ 1, A ^ 1)])) == []          # validate.py:18
    assert recs(ts.make_pools(3, [A, B], [(0, 2)], [(B, A)])) == [(0, 0, A, B)]      # the opposite direction is another link
    assert recs(ts.make_pools(3, [A, B], [(0, 2)], [(A ^ 1, B ^ 1)])) == [(0, 0, A, B)]
    assert recs(ts.make_pools(3, [A, B ^ 1], [(0, 2)], [(A, B)])) == [(0, 0, A, B ^ 1)]
    assert recs(ts.make_pools(3, [A, B ^ 1], [(0, 2)], [(B, A ^ 1)])) == []


def test_palindromic_link():
    # A+ -> A- is its own reverse complement; so is A- -> A+, which is another link
    p = ts.make_pools(1, [A, A ^ 1, A], [(0, 3)], [(A, A ^ 1)])
    assert recs(p) == [(0, 1, A ^ 1, A)]
    assert tm.degree(p).tolist() == [2]


def test_self_loop_counts_two_and_duplicates_count_again():
    p = ts.make_pools(3, [A, A, B], [(0, 3)], [(A, A), (A, B), (A, B), (B ^ 1, A ^ 1)])
    assert recs(p) == []
    assert tm.degree(p).tolist() == [2 + 3, 3, 0]
    assert tm.degree_text(p) == b"#node.id\tnode.degree\n1\t5\n2\t3\n3\t0\n"


def test_short_paths_and_path_boundaries():
    # p0 = (), p1 = (A), p2 = (A, C) unsupported, p3 = (B, C): the pairs (A, A) and (C, B) across the boundaries are none
    p = ts.make_pools(3, [A, A, C, B, C], [(0, 0), (0, 1), (1, 3), (3, 5)], [(B, C)])
    assert recs(p) == [(2, 0, A, C)]
    assert tm.validate_text(p) == b"[odgi::validate] error: the path p2 does not respect the graph topology: the link 1+,3+ is missing.\n"
    assert recs(ts.make_pools(3, [A, B], [(0, 1), (1, 2)], [])) == []


def test_orientation_in_the_text():
    p = ts.make_pools(3, [A ^ 1, C], [(0, 2)], [])
    assert tm.validate_text(p).endswith(b"the link 1-,3+ is missing.\n")


@pytest.mark.parametrize("sh", ts.SHAPES, ids=lambda s: s.name)
def test_shapes_are_what_they_claim(sh):
    p = sh.pools()
    r = tm.validate(p)
    got = list(zip(r["path"].tolist(), r["step"].tolist()))
    if sh.missing is not None:
        assert got == sh.missing
    else:
        assert len(got) == sh.n_missing and got[-1] == sh.last
    # what the shape says about itself holds for the pools
    for path in p.paths:
        assert int(path["steps_start"]) <= int(path["steps_end"]) <= len(p.steps)
    assert len(p.steps) == 0 or int(p.steps.max()) >> 1 < len(p.segs)


def test_shape_constants_are_the_kernels():
    assert ts.kernel_constants() == {"kThreads": ts.THREADS, "kPer": ts.PER, "kMaxGrid": ts.MAX_GRID, "kLinear": ts.LINEAR}
    assert ts.BIG_N > 2 * 1_000_000 and ts.BIG_N > ts.MAX_GRID * ts.TILE  # every grid-stride loop goes round more than once
    hub = ts.BY_NAME["hub_rows"].pools()
    rows = np.bincount(hub.links["from_"], minlength=6)
    assert rows[0] > ts.LINEAR + 1 and rows[2] == ts.LINEAR and rows[4] == ts.LINEAR + 1
    assert tm.degree(ts.BY_NAME["degree_hub"].pools())[0] > 65535
    n_scan = {name: 2 * len(ts.BY_NAME[name].pools().segs) + 1 for name in ts.ROWS}  # the entries of the row scan
    assert n_scan["rows_last_tile_one_short"] == ts.TILE - 1 and n_scan["rows_last_tile_of_one"] == ts.TILE + 1
    assert -(-n_scan["rows_past_a_spine_round"] // ts.TILE) > ts.THREADS


def test_new_symbols_are_in_the_built_library():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    want = {"flatgfa_validate", "flatgfa_missing_links_free", "flatgfa_validate_table", "flatgfa_degree", "flatgfa_degree_table"}
    assert want <= exported, sorted(want - exported)
    assert want <= set(_lib.SIGNATURES)
