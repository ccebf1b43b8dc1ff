"""tests/flatten_model.py against the reference's own bytes (tests/golden/flatten/*.flatten.txt, written by `slow_odgi flatten`:
make_flatten_golden.py), against hand-written cases at the FASTA's wrap, and its mirrored constants against the source."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import chop_shapes as cs
import flatten_model as fm
import random_pools as rp
from conftest import GOLDEN
from oracle import flatgfa_oracle as fo

FLAT = os.path.join(GOLDEN, "flatten")
with open(os.path.join(FLAT, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)


def golden_cases():
    """(stem, GFA path) of every *.flatten.txt in the directory: each must have its input, none is skipped."""
    out = []
    for txt in sorted(glob.glob(os.path.join(FLAT, "*.flatten.txt"))):
        stem = os.path.basename(txt)[:-len(".flatten.txt")]
        gfa = [g for g in (os.path.join(GOLDEN, stem + ".gfa"), os.path.join(FLAT, stem + ".gfa")) if os.path.exists(g)]
        assert len(gfa) == 1, stem
        out.append((stem, gfa[0]))
    return out


CASES = golden_cases()


def test_every_golden_is_listed():
    assert len(CASES) >= 14
    assert {s + ".flatten.txt" for s, _ in CASES} == {k for k in MANIFEST if k.endswith(".flatten.txt")}
    assert sum(1 for s, _ in CASES if MANIFEST[s + ".flatten.txt"]["input_ends_in_newline"]) >= 13


@pytest.mark.parametrize("stem,gfa", CASES, ids=[s for s, _ in CASES])
def test_model_is_the_reference(stem, gfa):
    with open(gfa, "rb") as f:
        text = f.read()
    with open(os.path.join(FLAT, stem + ".flatten.txt"), "rb") as f:
        want = f.read()
    assert hashlib.sha256(want).hexdigest() == MANIFEST[stem + ".flatten.txt"]["sha256"]
    # (mygfa reads an unterminated last line whole; so does the oracle's parser, memfile.rs:51-63)
    p = fo.parse_gfa(text)
    assert fm.flatten(p, stem.encode() + b".og") == want
    assert fm.bed_fast(p, stem.encode() + b".og") == fm.bed(p, stem.encode() + b".og")


@pytest.mark.parametrize("seed", rp.TEXT_SEEDS)
def test_model_is_the_reference_on_random_graphs(seed):
    """random_pools' text profile: sparse names, segments of one base, paths of one and two steps between long ones."""
    p = rp.make(seed, "text")
    assert hashlib.sha256(rp.gfa_text(p)).hexdigest() == MANIFEST["random_%d.gfa" % seed]["sha256"]  # the graph the reference was given
    with open(os.path.join(FLAT, "random_%d.flattened.txt" % seed), "rb") as f:
        want = f.read()
    assert hashlib.sha256(want).hexdigest() == MANIFEST["random_%d.flattened.txt" % seed]["sha256"]
    assert fm.flatten(p, b"random_%d.og" % seed) == want
    assert fm.bed_fast(p, b"random_%d.og" % seed) == fm.bed(p, b"random_%d.og" % seed)


def test_synth_flat_wraps_and_ranks():
    """What the synthetic graph is there for."""
    with open(os.path.join(FLAT, "synth_flat.gfa"), "rb") as f:
        p = fo.parse_gfa(f.read())
    assert fm.legend(p)[-1] > 24 * fm.WRAP
    assert len(p.paths) == 3 and all(int(q["steps_end"]) - int(q["steps_start"]) > 100 for q in p.paths)


def one_path(lens):
    return cs.make_pools(lens, [0], [(0, 1)])


@pytest.mark.parametrize("total,body", [(0, b"\n"), (1, b"A\n"), (79, b"A" * 79 + b"\n"), (80, b"A" * 80 + b"\n"),
                                        (81, b"A" * 80 + b"\nA\n"), (160, b"A" * 80 + b"\n" + b"A" * 80 + b"\n"),
                                        (161, b"A" * 80 + b"\n" + b"A" * 80 + b"\nA\n")])
def test_fasta_wrap_by_hand(total, body):
    p = one_path([total])
    assert fm.fasta(p, b"x") == b">x\n" + body
    assert fm.fasta_body_len(total) == len(body)
    # the rule the kernel uses: byte q is a newline when q % 81 == 80 or q is last, else base q - q // 81
    for q, ch in enumerate(body):
        assert (ch == 10) == (q % 81 == 80 or q == len(body) - 1)
        assert ch == 10 or q - q // 81 < total


def test_bed_by_hand():
    # segments of 3, 0 and 2 bases spelled out of order in seq_data; two paths over overlapping spans, one empty between
    p = cs.make_pools([3, 0, 2], [0, 3, 4, 5], [(0, 3), (2, 2), (1, 4)])
    p.seq_data = np.frombuffer(b"GTACC", np.uint8).copy()
    p.segs["seq_start"], p.segs["seq_end"] = [2, 2, 0], [5, 2, 2]
    assert fm.legend(p) == [0, 3, 3, 5]
    assert fm.fasta(p, b"n") == b">n\nACCGT\n"
    assert fm.bed(p, b"n") == (fm.BED_HEADER + b"n\t0\t3\tp\t+\t0\nn\t3\t3\tp\t-\t1\nn\t3\t5\tp\t+\t2\n"
                               b"n\t3\t3\tp\t-\t0\nn\t3\t5\tp\t+\t1\nn\t3\t5\tp\t-\t2\n")
    assert fm.bed(p, b"") .startswith(fm.BED_HEADER + b"\t0\t3\tp\t+\t0\n")


def test_mirrored_constants():
    c = fm.source_constants()
    assert c == {"TILE": fm.TILE, "PIECE": fm.PIECE, "THREADS": fm.THREADS, "SCAN_PER": fm.SCAN_PER, "CHUNK_LINES": fm.CHUNK_LINES,
                 "LONG_NAME": fm.LONG_NAME, "WRAP": fm.WRAP}
    assert fm.SCAN_TILE == c["THREADS"] * c["SCAN_PER"]
