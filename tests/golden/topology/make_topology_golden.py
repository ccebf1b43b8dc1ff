"""Regenerates the validate and degree goldens with the reference's own code: `slow_odgi validate`, `slow_odgi degree` and
`slow_odgi validate_setup` (validate_setup.drop_some_links: random.seed(4), 10 % of the links kept) -- the reference's
tests/turnt.toml validate and degree environments -- on every tests/golden/*.gfa:

    <name>.validate.txt  <name>.degree.tsv  <name>.dropped.gfa  <name>.dropped.validate.txt

and on the mid-size synthetic graph of tests/topology_shapes.py (synth_mid), whose GFA text is regenerated from its spec and
not kept: synth_mid.validate.txt, synth_mid.degree.tsv; and on three small random graphs (tests/random_pools.py, profile "text", seeds
TEXT_SEEDS: a quarter of the induced links dropped, each written in one spelling, duplicates in both spellings, self-loops, the
palindromic x+ -> x-, a hub row past the linear-probe threshold, sparse names), regenerated from the seed and not kept either:
random_<seed>.validate.txt, random_<seed>.degree.tsv.  mygfa splits a line on blanks and admits only ATGCN, so the text profile
has no empty segment; it has no path without steps and no path name that is empty or taken either.  MANIFEST.json records the sha256 of every output.  Needs the
reference's slow_odgi and mygfa on PYTHONPATH; the tests only read the outputs.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/topology/make_topology_golden.py
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


def slow_odgi(cmd, gfa):
    return subprocess.run([sys.executable, "-m", "slow_odgi", cmd, gfa], check=True, capture_output=True, timeout=1200).stdout


def main():
    manifest = {}

    def write(name, data):
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        manifest[name] = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data), "lines": data.count(b"\n")}

    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))):
        name = os.path.basename(gfa)[:-4]
        write(name + ".validate.txt", slow_odgi("validate", gfa))
        write(name + ".degree.tsv", slow_odgi("degree", gfa))
        write(name + ".dropped.gfa", slow_odgi("validate_setup", gfa))
        write(name + ".dropped.validate.txt", slow_odgi("validate", os.path.join(HERE, name + ".dropped.gfa")))
        print(name, manifest[name + ".validate.txt"]["lines"], manifest[name + ".dropped.validate.txt"]["lines"])

    import topology_shapes as ts
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "synth_mid.gfa")
        text = ts.gfa_text(ts.synth_mid())
        with open(path, "wb") as f:
            f.write(text)
        write("synth_mid.validate.txt", slow_odgi("validate", path))
        write("synth_mid.degree.tsv", slow_odgi("degree", path))
    manifest["synth_mid.gfa"] = {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "spec": ts.SYNTH_MID, "committed": False}
    print("synth_mid", manifest["synth_mid.validate.txt"])
    import random_pools as rp
    with tempfile.TemporaryDirectory() as d:
        for seed in rp.TEXT_SEEDS:
            stem = "random_%d" % seed
            text = rp.gfa_text(rp.make(seed, "text"))
            path = os.path.join(d, stem + ".gfa")
            with open(path, "wb") as f:
                f.write(text)
            write(stem + ".validate.txt", slow_odgi("validate", path))
            write(stem + ".degree.tsv", slow_odgi("degree", path))
            manifest[stem + ".gfa"] = {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "profile": "text", "seed": seed, "committed": False}
            print(stem, manifest[stem + ".validate.txt"]["lines"])
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
