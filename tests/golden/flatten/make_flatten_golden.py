"""Regenerates the flatten goldens with the reference's own code: `slow_odgi flatten` (slow_odgi/flatten.py, the reference's
tests/turnt.toml flatten environment) on every tests/golden/*.gfa and on one small synthetic graph, synth_flat.gfa, written
here by oracle/synth.py and kept: 300 segments and 3 paths of 120 steps, so that the FASTA wraps dozens of times and the
ranks pass 9/10 and 99/100.  The command runs from inside the graph's directory, so NAME is "<stem>.og" (__main__.py:178):

    <stem>.flatten.txt      the FASTA record, then the BED table

Three small random graphs (tests/random_pools.py, profile "text", seeds TEXT_SEEDS: sparse names, segments of one base, paths of one
and two steps between long ones) are flattened too, from a file named random_<seed>.gfa, so NAME is "random_<seed>.og"; their GFA
text is regenerated from the seed and not kept, and the outputs' names keep clear of *.flatten.txt, which
tests/test_flatten_model.py pairs with a committed input:

    random_<seed>.flattened.txt

mygfa splits a line on blanks and admits only ATGCN, so the text profile has no empty segment; it has no path without steps and no
path name that is empty or taken either (the reference keys paths by name).

MANIFEST.json records the sha256 and size of every output and whether its input ends in a newline (the reference's parser
and this project's read an unterminated last line differently; the tests hold the device against these bytes where it
does and against tests/flatten_model.py everywhere).  Needs the reference's slow_odgi and mygfa on PYTHONPATH; the tests only
read the outputs.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/flatten/make_flatten_golden.py
"""
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SYNTH_FLAT = {"seed": 11, "S": 300, "P": 3, "L": 120, "model": "pangenome"}


def slow_odgi_flatten(gfa):
    d, base = os.path.split(gfa)
    return subprocess.run([sys.executable, "-m", "slow_odgi", "flatten", base], check=True, capture_output=True, timeout=1200, cwd=d).stdout


def main():
    from oracle import synth
    text = synth.gfa_text(synth.pools(**SYNTH_FLAT))
    with open(os.path.join(HERE, "synth_flat.gfa"), "wb") as f:
        f.write(text)
    manifest = {"synth_flat.gfa": {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "spec": SYNTH_FLAT}}
    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))) + [os.path.join(HERE, "synth_flat.gfa")]:
        stem = os.path.basename(gfa)[:-4]
        out = slow_odgi_flatten(gfa)
        with open(gfa, "rb") as f:
            ends = f.read().endswith(b"\n")
        with open(os.path.join(HERE, stem + ".flatten.txt"), "wb") as f:
            f.write(out)
        manifest[stem + ".flatten.txt"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "lines": out.count(b"\n"),
                                           "input_ends_in_newline": ends}
        print(stem, len(out), ends)
    import random_pools as rp
    largest = max(v["bytes"] for v in manifest.values())
    with tempfile.TemporaryDirectory() as d:
        for seed in rp.TEXT_SEEDS:
            stem = "random_%d" % seed
            text = rp.gfa_text(rp.make(seed, "text"))
            with open(os.path.join(d, stem + ".gfa"), "wb") as f:
                f.write(text)
            out = slow_odgi_flatten(os.path.join(d, stem + ".gfa"))
            assert len(out) <= largest
            with open(os.path.join(HERE, stem + ".flattened.txt"), "wb") as f:
                f.write(out)
            manifest[stem + ".gfa"] = {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "profile": "text", "seed": seed, "committed": False}
            manifest[stem + ".flattened.txt"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "lines": out.count(b"\n")}
            print(stem, len(out))
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
