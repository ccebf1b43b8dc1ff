"""Pins tests/flip_model.py: its rules to hand-worked answers, its two forms of the de-duplication to each other (every shape of
tests/flip_shapes.py), and the model's text to the reference's own output (tests/golden/flip, made by make_flip_golden.py; its
files end in .txt because tests/test_parse_shapes.py counts every *.gfa under tests/golden).  The reference sorts its lines and
prints its links normalised, so the comparison is by views (crush_model.text_views), not by bytes.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import crush_model as cm
import flip_model as fm
import flip_shapes as fs
import pollen_amd as pa
import random_pools as rp
from conftest import GOLDEN, golden_gfas

FLIP = os.path.join(GOLDEN, "flip")
with open(os.path.join(FLIP, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
FIXTURES = golden_gfas() + [os.path.join(FLIP, "synth_flip.gfa.txt")]


h = fs.h


def stem_of(path):
    return os.path.basename(path).split(".")[0]


def test_constants_are_the_source_texts():
    assert fm.source_constants() == {"THREADS": fm.THREADS, "PER": fm.PER, "GRID": fm.GRID, "SCAN_PER": fm.SCAN_PER, "SHORT_ROW": fm.SHORT_ROW,
                                     "LDS_ROW": fm.LDS_ROW}
    assert fm.TILE == fm.THREADS * fm.PER and fm.SHORT_ROW == 64


# ---- rule 1 ----
def test_a_path_turns_iff_strictly_more_bases_walk_backward():
    p = fs.graph([3, 3, 7, 0], [[h(0), h(1, True)],            # a tie
                                [],                               # empty
                                [h(3, True), h(3, True)],         # empty segments only
                                [h(0), h(1), h(2, True)],         # 6 forward, 7 backward
                                [h(2), h(0, True), h(1, True)],   # 7 forward, 6 backward
                                [h(0, True)]])
    assert [fm.weigh(p, i) for i in range(6)] == [(3, 3), (0, 0), (0, 0), (6, 7), (7, 6), (0, 3)]
    assert fm.turned(p).tolist() == [False, False, False, True, False, True]


@pytest.mark.parametrize("name", list(fs.HEAVY))
def test_sums_past_32_bits(name):
    p = fs.HEAVY[name]()
    fwd, rev = fm.weigh(p, 0)
    assert {fwd, rev} == {(1 << 32) + (1 << 16), 1 << 31}
    assert bool(fm.turned(p)[0]) == (rev > fwd) == name.startswith("rev")
    assert ((rev & 0xFFFFFFFF) > (fwd & 0xFFFFFFFF)) != (rev > fwd)  # (what a 32-bit sum would say)


# ---- rules 2 to 4 ----
def test_steps_names_and_candidates_by_hand():
    p = fs.graph([1, 3, 1], [[h(0), h(1, True), h(2)], [h(0), h(1)]], names=[b"x", b"y"])  # ref_handmade_flip1's x, and one that stays
    t = fm.turned(p)
    assert t.tolist() == [True, False]
    steps = fm.new_steps(p, t)
    assert steps[0].tolist() == [h(2, True), h(1), h(0, True)] and steps[1].tolist() == [h(0), h(1)]
    assert fm.new_names(p, t) == [b"x_inv", b"y"]
    assert fm.candidates(steps, t) == [(h(2, True), h(1)), (h(1), h(0, True))]
    q = fm.flip(p)
    assert q.name_data.tobytes() == b"x_invy" and [(int(r["name_start"]), int(r["name_end"])) for r in q.paths] == [(0, 5), (5, 6)]
    assert [(int(r["steps_start"]), int(r["steps_end"])) for r in q.paths] == [(0, 3), (3, 5)] and not q.paths["ov_end"].any()
    assert q.alignment.tolist() == [fm.ZERO_M] and [tuple(int(x) for x in r) for r in q.links] == [(h(2, True), h(1), 0, 1), (h(1), h(0, True), 0, 1)]


# ---- rule 5 ----
M0, M5 = (fs.op(0),), (fs.op(5),)
DEDUP = [
    ([(2, 4, M0), (2, 4, M0)], [0]),                                 # verbatim
    ([(2, 4, M0), (5, 3, M0)], [0]),                                 # as its reverse
    ([(2, 4, M5), (2, 4, M0)], [0, 1]),                              # the overlap takes part
    ([(2, 4, M5), (5, 3, M0), (5, 3, M5)], [0, 1]),
    ([(2, 3, M0), (2, 3, M0)], [0]),                                 # palindromic: its own reverse
    ([(2, 2, M0), (3, 3, M0), (2, 2, M0)], [0]),                     # a self-loop and its reverse
    ([(2, 4, ()), (2, 4, M0), (5, 3, ())], [0, 1]),                  # an empty overlap is not 0M
    ([(2, 4, (fs.op(3), fs.op(1, 2))), (2, 4, (fs.op(3), fs.op(1, 3))), (5, 3, (fs.op(3), fs.op(1, 2)))], [0, 1]),
    ([(6, 8, M0), (2, 4, M0), (9, 7, M0), (4, 2, M0)], [0, 1, 3]),   # order is kept; 4 -> 2 is not 2 -> 4
]


@pytest.mark.parametrize("links,want", DEDUP)
def test_dedup_by_hand(links, want):
    assert fm.dedup(links) == want and fm.dedup_fast(links) == want


def test_old_links_are_deduplicated_when_no_path_turns():
    p = fs.graph([1, 1, 1], [[h(0), h(1)]], [(h(0), h(1), [fs.op(0)]), (h(1, True), h(0, True), [fs.op(0)]), (h(0), h(1), [fs.op(5)])])
    q = fm.flip(p)
    assert not fm.turned(p).any() and len(q.links) == 2 and q.alignment.tobytes() == p.alignment.tobytes()
    assert q.links.tobytes() == p.links[[0, 2]].tobytes()  # (the old spans)


def test_a_candidate_under_an_old_link_of_another_overlap_stays_beside_it():
    p = fs.graph([1, 1], [[h(1, True), h(0, True)]], [(h(0), h(1), [fs.op(5)])])
    q = fm.flip(p)
    assert [tuple(int(x) for x in r) for r in q.links] == [(h(0), h(1), 0, 1), (h(0), h(1), 1, 2)] and q.alignment.tolist() == [fs.op(5), 0]


def test_flip_of_flip_is_flip():
    for name in ("paths of T-1, T, T+1, 2T+1 steps, every other turned", "gapped, overlapping and out-of-order spans", "rows of SHORT+1 and SHORT-1 keys"):
        q = fm.flip(fs.SHAPES[name]())
        assert not fm.turned(q).any()
        fm.assert_same_pools(fm.flip(q), q, name)


@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_shapes(name):
    p = fs.SHAPES[name]()
    q = fm.flip(p)
    if len(p.links) + len(p.steps) < 20000:
        fm.assert_same_pools(fm.flip(p, fast=False), q, name)
    rows = fm.row_sizes(p)
    if name.startswith("rows of"):
        base = fm.SHORT_ROW if "SHORT" in name else fm.LDS_ROW
        d = int(name.split()[2][len("SHORT" if "SHORT" in name else "LDS"):])
        assert rows[h(0)] == base + d and rows[h(0, True)] == base + d - 2
        assert len(q.links) < len(p.links) + rows[h(0)] + rows[h(0, True)] - 5  # (old links and candidates both lose some)
    if name == "one pair 10^5 times":
        assert max(rows.values()) == 100000 and len(q.links) == 2
    if "every other turned" in name:
        assert fm.turned(p).tolist() == [True, False, True, False]
    if name.startswith("a turned path"):
        assert fm.turned(p).tolist() == [False, True, False]
    assert int(q.paths["steps_end"][-1]) == len(q.steps) if len(q.paths) else len(q.steps) == 0


def test_what_is_refused():
    ok = fs.graph([2, 2], [[h(0), h(1, True)]], [(h(0), h(1), [fs.op(0)])])
    fm.flip(ok)
    for field, arr, at, value in [("steps", "steps", 0, h(2)), ("links", "links", 0, (h(2), 0, 0, 1)), ("links", "links", 0, (0, 2, 0, 2)),
                                  ("links", "links", 0, (0, 2, 1, 0)), ("paths", "paths", 0, (0, 2, 1, 3, 0, 0)), ("segs", "segs", 1, (2, 2, 5, 0, 0))]:
        p = fs.graph([2, 2], [[h(0), h(1, True)]], [(h(0), h(1), [fs.op(0)])])
        getattr(p, arr)[at] = value
        with pytest.raises(IndexError):
            fm.flip(p)


# ---- the reference's own output ----
@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_model_text_is_the_references(path):
    stem = stem_of(path)
    rec = MANIFEST[stem + ".flip.gfa.txt"]
    with open(os.path.join(FLIP, stem + ".flip.gfa.txt"), "rb") as f:
        ref = f.read()
    assert hashlib.sha256(ref).hexdigest() == rec["sha256"] and len(ref) == rec["bytes"]
    g = pa.parse(path)
    p = fm.pools_of(g)
    g.close()
    q = fm.flip(p)
    fm.assert_same_pools(q, fm.flip(p, fast=False), stem)
    if not rec["input_ends_in_newline"]:  # (the two parsers read an unterminated last line differently: the model only)
        return
    assert fm.counts(p) == (rec["turned"], rec["links_out"]) and len(p.links) == rec["links_in"]
    got = cm.text_views(fm.text(q), ours=True)
    want = cm.text_views(ref)
    for a, b, what in zip(got, want, ("S", "P", "L", "H")):
        assert a == b, (stem, what)


@pytest.mark.parametrize("seed", rp.TEXT_SEEDS)
def test_model_text_is_the_references_on_random_graphs(seed):
    """random_pools' text profile: ties, twins, self-loops, x+ -> x-, old links in both spellings and with 5M, a hub row."""
    p = rp.make(seed, "text")
    src = MANIFEST["random_%d.gfa" % seed]
    assert hashlib.sha256(rp.gfa_text(p)).hexdigest() == src["sha256"]  # the graph the reference was given
    rec = MANIFEST["random_%d.flip.txt" % seed]
    with open(os.path.join(FLIP, "random_%d.flip.txt" % seed), "rb") as f:
        ref = f.read()
    assert hashlib.sha256(ref).hexdigest() == rec["sha256"] and len(ref) == rec["bytes"]
    q = fm.flip(p)
    fm.assert_same_pools(q, fm.flip(p, fast=False), seed)
    assert fm.counts(p) == (rec["turned"], rec["links_out"]) and len(p.links) == rec["links_in"] and rec["turned"] >= 3
    for a, b, what in zip(cm.text_views(fm.text(q), ours=True), cm.text_views(ref), ("S", "P", "L", "H")):
        assert a == b, (seed, what)


def test_the_goldens_turn_paths_and_add_links():
    recs = {k[:-len(".flip.gfa.txt")]: v for k, v in MANIFEST.items() if k.endswith(".flip.gfa.txt")}
    assert len(recs) == 14
    table = {"edge_names_loops": (1, 4, 4), "kat_window_depth": (1, 0, 0), "ref_handmade_flip1": (1, 2, 4), "ref_handmade_flip2": (2, 2, 4),
             "ref_handmade_flip3": (1, 20, 23), "standin_note5": (1, 4, 4)}
    for stem, want in table.items():
        assert (recs[stem]["turned"], recs[stem]["links_in"], recs[stem]["links_out"]) == want, stem
    assert all(v["turned"] == 0 for k, v in recs.items() if k not in table and k != "synth_flip")
    assert recs["synth_flip"]["turned"] >= 10 and recs["synth_flip"]["links_out"] > recs["synth_flip"]["links_in"]


def test_the_synthetic_graph_holds_what_it_must():
    g = pa.parse(os.path.join(FLIP, "synth_flip.gfa.txt"))
    p = fm.pools_of(g)
    g.close()
    names = fm.new_names(p, np.zeros(len(p.paths), bool))
    assert len(set(names)) == len(names) and 200 <= len(p.segs) <= 400
    t = dict(zip(names, fm.turned(p).tolist()))
    assert not t[b"tie"] and fm.weigh(p, names.index(b"tie"))[0] == fm.weigh(p, names.index(b"tie"))[1] > 0
    assert t[b"one"] and t[b"two"] and t[b"opp_a"] and t[b"opp_b"] and t[b"loop"] and t[b"pal"] and t[b"shadowed"] and t[b"again"]
    steps = dict(zip(names, fm.new_steps(p, fm.turned(p))))
    assert len(steps[b"one"]) == 1 and len(steps[b"two"]) == 2
    seg = {int(s["name"]): i for i, s in enumerate(p.segs)}
    hh = lambda name, back=False: h(seg[name], back)  # noqa: E731
    a, b = tuple(steps[b"opp_a"].tolist()), tuple(steps[b"opp_b"].tolist()[1:])
    assert a == (hh(9), hh(10)) and b == (hh(10, True), hh(9, True)) and fm.rev(a + ((),))[:2] == b  # one link, from opposite ends
    assert steps[b"loop"].tolist() == [hh(14), hh(14)] and steps[b"pal"].tolist()[1:] == [hh(16), hh(16, True)]
    old = fm.old_links(p)
    assert old.count((hh(20), hh(21), M0)) == 2 and (hh(21, True), hh(20, True), M0) in old       # verbatim, and as its reverse
    assert (hh(8), hh(7), M5) in old and tuple(steps[b"two"].tolist()) == (hh(8), hh(7))            # 5M under a candidate's pair
    assert (hh(30, True), hh(31, True), M0) in old and tuple(steps[b"shadowed"].tolist()) == (hh(31), hh(30))
    q = fm.flip(p)
    kept = [(int(r["from_"]), int(r["to"]), tuple(int(x) for x in q.alignment[int(r["ov_start"]):int(r["ov_end"])])) for r in q.links]
    assert kept.count((hh(8), hh(7), M5)) == 1 and kept.count((hh(8), hh(7), M0)) == 1
    assert kept.count((hh(9), hh(10), M0)) + kept.count((hh(10, True), hh(9, True), M0)) == 1
    assert (hh(31), hh(30), M0) not in kept and kept.count((hh(14), hh(14), M0)) == 1 and kept.count((hh(16), hh(16, True), M0)) == 1
