"""Regenerates the flip goldens with the reference's own code: `slow_odgi flip` (slow_odgi/flip.py) on every
tests/golden/*.gfa and on one small synthetic graph, synth_flip.gfa.txt, written here and kept: 300 segments, unique path names,
and planted by hand, beside twelve seeded random walks of which about half turn:

    tie                 1+,1-: as many bases backward as forward -- stays
    one                 5-: turns, and has no pair
    two                 7-,8-: turns into 8+,7+; the old link 8+ -> 7+ has the overlap 5M, so the 0M candidate stays beside it
    opp_a, opp_b        10-,9- and 9+,10+,12- (segment 12 is long): their new steps need 9+ -> 10+ and 10- -> 9-, one link
    loop                14-,14-: the self-loop 14+ -> 14+
    pal                 16+,16-,17- (segment 17 is long): the new steps 17+,16+,16- need the palindromic link 16+ -> 16-,
                        which is its own reverse
    shadowed            30-,31-: needs 31+ -> 30+, which the old link 30- -> 31- (0M) is already, as its reverse
    again               30-,31- once more, under another name
    old links           20+ -> 21+ three times over: verbatim twice and once as 21- -> 20-; the same pair once more with 3M1D,
                        twice; an old palindromic link 40+ -> 40-; an old self-loop 41+ -> 41+ twice

    <stem>.flip.gfa.txt   the graph as the reference prints it (links normalised, lines sorted)

(The names end in .txt because tests/test_parse_shapes.py counts every *.gfa under tests/golden.)

Three small random graphs (tests/random_pools.py, profile "text", seeds TEXT_SEEDS: ties of the two weights, one pair walked by two
turned paths and by a path that stays, self-loops, the palindromic x+ -> x-, old links in both spellings and with 5M beside 0M, a hub
row, sparse names) are flipped too; their GFA text is regenerated from the seed and not kept:

    random_<seed>.flip.txt

mygfa splits a line on blanks and admits only ATGCN, so the text profile has no empty segment; it has no path without steps and no
path name that is empty or taken either (the reference keys paths by name).  The palindromic link x- -> x+ is left out as well, as a
link and as a pair of steps, which flip would make one: mygfa's Link.__str__ (gfa.py:196-201) reverses it into itself without end.

MANIFEST.json records the sha256 and size of every output, how many paths turned (the P lines named `_inv` that the input
does not have), the L lines of the input and of the output, and whether the input ends in a newline (the reference's parser
and this project's read an unterminated last line differently; the tests hold the device against these bytes where it does
and against tests/flip_model.py everywhere).  Needs the reference's slow_odgi and mygfa on PYTHONPATH; the tests only read
the outputs.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/flip/make_flip_golden.py
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

SYNTH_FLIP = {"seed": 23, "S": 300, "walks": 12, "L": 60, "links": 40}

PLANTED_PATHS = [
    (b"tie", b"1+,1-"), (b"one", b"5-"), (b"two", b"7-,8-"), (b"opp_a", b"10-,9-"), (b"opp_b", b"9+,10+,12-"), (b"loop", b"14-,14-"),
    (b"pal", b"16+,16-,17-"), (b"shadowed", b"30-,31-"), (b"again", b"30-,31-"),
]
PLANTED_LINKS = [
    b"8\t+\t7\t+\t5M", b"30\t-\t31\t-\t0M", b"20\t+\t21\t+\t0M", b"20\t+\t21\t+\t0M", b"21\t-\t20\t-\t0M", b"20\t+\t21\t+\t3M1D",
    b"21\t-\t20\t-\t3M1D", b"40\t+\t40\t-\t0M", b"41\t+\t41\t+\t0M", b"41\t+\t41\t+\t0M",
]
LONG = {12: 90, 17: 90}  # (segments whose one backward step outweighs the forward ones before it)


def synth_text(seed, S, walks, L, links):
    rng = np.random.default_rng(seed)
    lines = [b"H\tVN:Z:1.0"]
    for i in range(1, S + 1):
        n = LONG.get(i, int(rng.integers(1, 41)))
        lines.append(b"S\t%d\t%s" % (i, bytes(int(c) for c in rng.choice(list(b"ACGT"), n))))
    o = lambda: b"+-"[int(rng.integers(0, 2)):][:1]  # noqa: E731
    for k in range(walks):
        # a walk over segments 100..: a few steps repeat, so that a turned walk needs one link more than once
        segs = [int(rng.integers(100, S + 1)) for _ in range(L)]
        segs[10:14] = segs[2:6]
        ori = [o() for _ in range(L)]
        ori[10:14] = ori[2:6]
        lines.append(b"P\twalk%d\t" % k + b",".join(b"%d%s" % (s, c) for s, c in zip(segs, ori)) + b"\t*")
    lines += [b"P\t%s\t%s\t*" % (n, s) for n, s in PLANTED_PATHS]
    seen = set()
    while len(seen) < links:
        ln = (int(rng.integers(100, S + 1)), o(), int(rng.integers(100, S + 1)), o())
        if ln not in seen:
            seen.add(ln)
            lines.append(b"L\t%d\t%s\t%d\t%s\t0M" % ln)
    lines += [b"L\t" + ln for ln in PLANTED_LINKS]
    return b"\n".join(lines) + b"\n"


def slow_odgi_flip(gfa):
    d, base = os.path.split(gfa)
    return subprocess.run([sys.executable, "-m", "slow_odgi", "flip", base], check=True, capture_output=True, timeout=1200, cwd=d).stdout


def lines_of(text, kind):
    return [ln for ln in text.splitlines() if ln[:1] == kind]


def main():
    text = synth_text(**SYNTH_FLIP)
    with open(os.path.join(HERE, "synth_flip.gfa.txt"), "wb") as f:
        f.write(text)
    manifest = {"synth_flip.gfa.txt": {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "spec": SYNTH_FLIP}}
    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))) + [os.path.join(HERE, "synth_flip.gfa.txt")]:
        stem = os.path.basename(gfa).split(".")[0]
        out = slow_odgi_flip(gfa)
        with open(gfa, "rb") as f:
            src = f.read()
        with open(os.path.join(HERE, stem + ".flip.gfa.txt"), "wb") as f:
            f.write(out)
        names_in = {ln.split(b"\t")[1] for ln in lines_of(src, b"P")}
        turned = sum(1 for ln in lines_of(out, b"P") if ln.split(b"\t")[1].endswith(b"_inv") and ln.split(b"\t")[1] not in names_in)
        manifest[stem + ".flip.gfa.txt"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "turned": turned,
                                        "links_in": len(lines_of(src, b"L")), "links_out": len(lines_of(out, b"L")),
                                        "input_ends_in_newline": src.endswith(b"\n")}
        print(stem, len(out), turned, manifest[stem + ".flip.gfa.txt"]["links_in"], manifest[stem + ".flip.gfa.txt"]["links_out"])
    import random_pools as rp
    largest = max(v["bytes"] for v in manifest.values())
    with tempfile.TemporaryDirectory() as d:
        for seed in rp.TEXT_SEEDS:
            stem = "random_%d" % seed
            text = rp.gfa_text(rp.make(seed, "text"))
            with open(os.path.join(d, stem + ".gfa"), "wb") as f:
                f.write(text)
            out = slow_odgi_flip(os.path.join(d, stem + ".gfa"))
            assert len(out) <= largest
            with open(os.path.join(HERE, stem + ".flip.txt"), "wb") as f:
                f.write(out)
            turned = sum(1 for ln in lines_of(out, b"P") if ln.split(b"\t")[1].endswith(b"_inv"))
            manifest[stem + ".gfa"] = {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "profile": "text", "seed": seed, "committed": False}
            manifest[stem + ".flip.txt"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "turned": turned,
                                            "links_in": len(lines_of(text, b"L")), "links_out": len(lines_of(out, b"L"))}
            print(stem, len(out), turned, len(lines_of(text, b"L")), len(lines_of(out, b"L")))
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
