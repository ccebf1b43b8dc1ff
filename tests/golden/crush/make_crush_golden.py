"""Regenerates the crush goldens with the reference's own code: `slow_odgi crush` (slow_odgi/crush.py) on every
tests/golden/*.gfa and on one small synthetic graph, synth_crush.gfa, written here and kept: 300 segments with N planted by a
seeded rule -- runs of length 1, 2 and 3 or more; at a segment's start, at its end, inside it and over all of it; and
neighbouring segments that end and start with N, whose runs must not join -- 3 paths and 40 links.

    <stem>.crush.gfa      the graph as the reference prints it

Three small random graphs (tests/random_pools.py, profile "text", seeds TEXT_SEEDS: N runs at segment ends and starts and on both
sides of a seam, sparse names, ties, palindromes, hub rows) are crushed too.  Their GFA text is regenerated from the seed and not
kept, and the outputs end in .txt because tests/test_parse_shapes.py counts every *.gfa under tests/golden:

    random_<seed>.crush.txt

mygfa splits a line on blanks and admits only ATGCN, so the text profile has no empty segment; it has no path without steps and no
path name that is empty or taken either (the reference keys paths by name and prints steps[0]).  The palindromic link x- -> x+ is left
out as well, as a link and as a pair of steps: mygfa's Link.__str__ (gfa.py:196-201) reverses it into itself without end.

MANIFEST.json records the sha256 and size of every output, how many bases the crush dropped (the S lines of the input and
of the output, compared) and whether the input ends in a newline (the reference's parser and this project's read an
unterminated last line differently; the tests hold the device against these bytes where it does and against
tests/crush_model.py everywhere).  Needs the reference's slow_odgi and mygfa on PYTHONPATH; the tests only read the outputs.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/crush/make_crush_golden.py
"""
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SYNTH_CRUSH = {"seed": 17, "S": 300, "P": 3, "L": 60, "links": 40}


def synth_text(seed, S, P, L, links):
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(S):
        n = int(rng.integers(1, 41))
        seq = bytearray(int(c) for c in rng.choice(list(b"ACGT"), n))
        kind = i % 10
        run = (1, 2, 3, 7)[(i // 10) % 4]
        if kind == 1:    # at the start
            seq[:0] = b"N" * run
        elif kind == 2:  # at the end
            seq += b"N" * run
        elif kind == 3:  # inside, twice
            at = int(rng.integers(0, len(seq) + 1))
            seq[at:at] = b"N" * run
            at = int(rng.integers(0, len(seq) + 1))
            seq[at:at] = b"N" * (run + 1)
        elif kind == 4:  # all of it
            seq = bytearray(b"N" * run)
        elif kind == 5:  # ends in N, and the next one (kind 6) starts with N
            seq += b"N" * run
        elif kind == 6:
            seq[:0] = b"N" * (run + 2)
        seqs.append(bytes(seq))
    lines = [b"H\tVN:Z:1.0"]
    lines += [b"S\t%d\t%s" % (i + 1, s) for i, s in enumerate(seqs)]
    o = lambda: b"+-"[int(rng.integers(0, 2)):][:1]  # noqa: E731
    for k in range(P):
        lines.append(b"P\tpath%d\t" % k + b",".join(b"%d%s" % (int(rng.integers(1, S + 1)), o()) for _ in range(L)) + b"\t*")
    seen = set()
    while len(seen) < links:
        ln = (int(rng.integers(1, S + 1)), o(), int(rng.integers(1, S + 1)), o())
        if ln not in seen:
            seen.add(ln)
            lines.append(b"L\t%d\t%s\t%d\t%s\t0M" % ln)
    return b"\n".join(lines) + b"\n"


def slow_odgi_crush(gfa):
    d, base = os.path.split(gfa)
    return subprocess.run([sys.executable, "-m", "slow_odgi", "crush", base], check=True, capture_output=True, timeout=1200, cwd=d).stdout


def bases(text):
    return sum(len(ln.split(b"\t")[2]) for ln in text.splitlines() if ln[:1] == b"S")


def main():
    text = synth_text(**SYNTH_CRUSH)
    with open(os.path.join(HERE, "synth_crush.gfa"), "wb") as f:
        f.write(text)
    manifest = {"synth_crush.gfa": {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "spec": SYNTH_CRUSH}}
    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))) + [os.path.join(HERE, "synth_crush.gfa")]:
        stem = os.path.basename(gfa)[:-4]
        out = slow_odgi_crush(gfa)
        with open(gfa, "rb") as f:
            src = f.read()
        with open(os.path.join(HERE, stem + ".crush.gfa"), "wb") as f:
            f.write(out)
        manifest[stem + ".crush.gfa"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "dropped": bases(src) - bases(out),
                                         "input_ends_in_newline": src.endswith(b"\n")}
        print(stem, len(out), manifest[stem + ".crush.gfa"]["dropped"])
    import random_pools as rp
    largest = max(v["bytes"] for v in manifest.values())
    with tempfile.TemporaryDirectory() as d:
        for seed in rp.TEXT_SEEDS:
            stem = "random_%d" % seed
            text = rp.gfa_text(rp.make(seed, "text"))
            with open(os.path.join(d, stem + ".gfa"), "wb") as f:
                f.write(text)
            out = slow_odgi_crush(os.path.join(d, stem + ".gfa"))
            assert len(out) <= largest
            with open(os.path.join(HERE, stem + ".crush.txt"), "wb") as f:
                f.write(out)
            manifest[stem + ".gfa"] = {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "profile": "text", "seed": seed, "committed": False}
            manifest[stem + ".crush.txt"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "dropped": bases(text) - bases(out)}
            print(stem, len(out), bases(text) - bases(out))
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
