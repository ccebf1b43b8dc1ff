"""Pins tests/crush_model.py: its two forms to each other (seeded random pools with planted runs, and every shape of
tests/crush_shapes.py), both to hand-worked answers, and the model's text to the reference's own output
(tests/golden/crush, made by make_crush_golden.py).  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import crush_model as cm
import crush_shapes as cs
import pollen_amd as pa
import random_pools as rp
from conftest import GOLDEN, fixture_id, golden_gfas

CRUSH = os.path.join(GOLDEN, "crush")
with open(os.path.join(CRUSH, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
FIXTURES = golden_gfas() + [os.path.join(CRUSH, "synth_crush.gfa")]


def test_constants_are_the_source_texts():
    assert cm.source_constants() == {"TILE": cm.TILE, "THREADS": cm.THREADS, "GRID": cm.GRID, "SCAN_PER": cm.SCAN_PER}
    assert cm.TILE // 64 == cm.THREADS


HAND = [
    (b"", b""), (b"N", b"N"), (b"NN", b"N"), (b"ANNA", b"ANA"), (b"NNNN", b"N"), (b"NAN", b"NAN"), (b"nnNN**", b"nnN**"),
    (b"NNANNNNCTGGAGNNCTAT", b"NANCTGGAGNCTAT"),  # ref_handmade_crush1, segment 9
    (b"ACGT", b"ACGT"), (b"NNNANNN", b"NAN"),
]


@pytest.mark.parametrize("seq,want", HAND)
def test_hand_worked_sequences(seq, want):
    assert cm.crush_seq(seq) == want
    for f in (cm.crush, cm.crush_fast):
        q = f(cs.of_seqs([b"AN", seq, b"NC"]))  # (between neighbours that end and start with N: runs do not join)
        assert q.seq_data.tobytes() == b"AN" + want + b"NC"
        assert [(int(s["seq_start"]), int(s["seq_end"])) for s in q.segs] == [(0, 2), (2, 2 + len(want)), (2 + len(want), 4 + len(want))]


def test_crush1_by_hand():
    g = pa.parse(os.path.join(GOLDEN, "ref_handmade_crush1.gfa"))
    p = cm.pools_of(g)
    q = cm.crush(p)
    seqs = {int(s["name"]): q.seq_data[int(s["seq_start"]):int(s["seq_end"])].tobytes() for s in q.segs}
    assert seqs[9] == b"NANCTGGAGNCTAT" and seqs[4] == b"N" and seqs[5] == b"N" and seqs[6] == b"NG"
    assert cm.dropped(p) == 12
    # the layout: one behind another in segment order; what is not the sequences' is kept or empty
    assert np.array_equal(q.segs["seq_start"][1:], q.segs["seq_end"][:-1]) and int(q.segs["seq_end"][-1]) == len(q.seq_data)
    assert not q.segs["opt_start"].any() and not q.segs["opt_end"].any() and not q.paths["ov_end"].any()
    for n in ("header", "steps", "links", "alignment", "name_data"):
        assert getattr(q, n).tobytes() == getattr(p, n).tobytes()
    assert len(q.overlaps) == 0 and len(q.optional_data) == 0 and len(q.line_order) == 0
    g.close()


def random_pools(seed):
    """Spans of every kind -- in order, out of order, overlapping, aliased, empty -- over a pool with planted runs."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 400))
    pool = np.frombuffer(b"ACGTn*", np.uint8)[rng.integers(0, 6, n)].copy()
    for _ in range(int(rng.integers(0, 12))):
        if n:
            at = int(rng.integers(0, n))
            pool[at:at + int(rng.integers(1, 9))] = cm.N
    S = int(rng.integers(0, 40))
    if seed % 3 == 0:  # tiling, in order, cut inside the runs too
        cuts = np.sort(rng.integers(0, n + 1, S + 1)) if S else np.zeros(1, np.int64)
        spans = [(int(cuts[i]), int(cuts[i + 1])) for i in range(S)]
    else:
        spans = []
        for _ in range(S):
            a = int(rng.integers(0, n + 1))
            spans.append((a, int(rng.integers(a, min(n, a + 60) + 1))))
        if S > 2:
            spans[1] = spans[0]
    return cs.pools(pool, spans)


@pytest.mark.parametrize("block", range(8))
def test_two_forms_agree_and_crush_is_idempotent(block):
    for seed in range(block * 40, block * 40 + 40):
        p = random_pools(seed)
        a, b = cm.crush(p), cm.crush_fast(p)
        cm.assert_same_pools(a, b, seed)
        cm.assert_same_pools(cm.crush_fast(a), a, seed)
        assert cm.dropped(a) == 0
        assert len(p.segs) == 0 or int(a.segs["seq_end"][-1]) == len(a.seq_data)


@pytest.mark.parametrize("name", list(cs.SHAPES))
def test_shapes(name):
    p = cs.SHAPES[name]()
    b = cm.crush_fast(p)
    if len(p.segs) < 20000 and len(p.seq_data) < 200000:
        cm.assert_same_pools(cm.crush(p), b, name)
    lens = (p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"]).sum()
    assert cm.dropped(p) == lens - len(b.seq_data)
    if "N on both sides" in name or name.startswith("single N"):
        assert cm.dropped(p) == 0 and b.seq_data.tobytes().count(b"NN") >= 1
    if name.startswith("3T+5"):
        assert cm.dropped(p) == 3 * cs.T + 4
    if name.startswith("kept bytes end"):
        assert len(b.seq_data) % 16 == int(name[-2:]) % 16
    if name == "more tiles than workgroups":
        assert lens > cm.GRID * cm.TILE


def test_spans_outside_the_pool_are_refused():
    with pytest.raises(IndexError):
        cm.crush(cs.pools(b"ACGT", [(0, 4), (2, 5)]))
    with pytest.raises(IndexError):
        cm.crush_fast(cs.pools(b"ACGT", [(3, 2)]))


# ---- the reference's own output ----
@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_model_text_is_the_references(path):
    stem = fixture_id(path)
    rec = MANIFEST[stem + ".crush.gfa"]
    with open(os.path.join(CRUSH, stem + ".crush.gfa"), "rb") as f:
        ref = f.read()
    assert hashlib.sha256(ref).hexdigest() == rec["sha256"] and len(ref) == rec["bytes"]
    g = pa.parse(path)
    p = cm.pools_of(g)
    g.close()
    q = cm.crush(p)
    cm.assert_same_pools(q, cm.crush_fast(p), stem)
    if not rec["input_ends_in_newline"]:  # (the two parsers read an unterminated last line differently: the model only)
        return
    assert cm.dropped(p) == rec["dropped"]
    got = cm.text_views(cm.text(q), ours=True)
    want = cm.text_views(ref)
    for a, b, what in zip(got, want, ("S", "P", "L", "H")):
        assert a == b, (stem, what)


@pytest.mark.parametrize("seed", rp.TEXT_SEEDS)
def test_model_text_is_the_references_on_random_graphs(seed):
    """random_pools' text profile: N on both sides of a seam, runs at segment ends, segments of one N, sparse names."""
    p = rp.make(seed, "text")
    src = MANIFEST["random_%d.gfa" % seed]
    assert hashlib.sha256(rp.gfa_text(p)).hexdigest() == src["sha256"]  # the graph the reference was given
    rec = MANIFEST["random_%d.crush.txt" % seed]
    with open(os.path.join(CRUSH, "random_%d.crush.txt" % seed), "rb") as f:
        ref = f.read()
    assert hashlib.sha256(ref).hexdigest() == rec["sha256"] and len(ref) == rec["bytes"]
    q = cm.crush(p)
    cm.assert_same_pools(q, cm.crush_fast(p), seed)
    assert cm.dropped(p) == rec["dropped"] > 50
    for a, b, what in zip(cm.text_views(cm.text(q), ours=True), cm.text_views(ref), ("S", "P", "L", "H")):
        assert a == b, (seed, what)


def test_at_least_two_fixtures_drop_bytes():
    drops = {k: v["dropped"] for k, v in MANIFEST.items() if k.endswith(".crush.gfa")}
    assert len(drops) == 14
    assert sum(1 for v in drops.values() if v > 0) >= 2 and drops["ref_handmade_crush1.crush.gfa"] == 12 and drops["synth_crush.crush.gfa"] > 100
