"""Regenerates the inject goldens with the reference's own code: `slow_odgi inject_setup` (inject_setup.py: up to five seeded
intervals per path) and `slow_odgi inject --bed` (inject.py) on every tests/golden/*.gfa whose segments are named 1..S in
file order -- slow_odgi's inject renumbers by numeric name, so only those come out in this project's order -- and on one small
synthetic graph, synth_inject.gfa, written here and kept: 300 segments, 6 paths of 80 steps, a third of them backward.

    <stem>.inject.bed      what inject_setup prints
    <stem>.inject.gfa      what inject --bed prints (H, S, P lines; slow_odgi prints no links for inject)

MANIFEST.json records the sha256 and size of every output, how many BED lines there are, how many segments the reference cut
(new segments minus old) and how many paths it added, and lists the fixtures that were left out and why.  A fixture with no
cut checks the new paths only.  Needs the reference's slow_odgi and mygfa on PYTHONPATH; the tests only read the outputs.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/inject/make_inject_golden.py
"""
import glob
import hashlib
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)

SYNTH = {"seed": 16, "S": 300, "P": 6, "L": 80}


def synth_text():
    rng = random.Random(SYNTH["seed"])
    lines = ["H\tVN:Z:1.0"]
    for s in range(SYNTH["S"]):
        lines.append("S\t%d\t%s" % (s + 1, "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 12)))))
    for p in range(SYNTH["P"]):
        at = rng.randrange(SYNTH["S"])
        steps = []
        for _ in range(SYNTH["L"]):
            steps.append("%d%s" % (at + 1, "-" if rng.random() < 0.33 else "+"))
            at = (at + rng.randint(1, 3)) % SYNTH["S"] if rng.random() < 0.9 else rng.randrange(SYNTH["S"])
        lines.append("P\tsyn%d\t%s\t*" % (p, ",".join(steps)))
    return ("\n".join(lines) + "\n").encode()


def slow_odgi(args, gfa):
    d, base = os.path.split(gfa)
    return subprocess.run([sys.executable, "-m", "slow_odgi"] + args + [base], check=True, capture_output=True, timeout=1200, cwd=d).stdout


def named_in_order(text):
    names = [ln.split(b"\t")[1] for ln in text.split(b"\n") if ln.startswith(b"S\t")]
    return names == [b"%d" % (i + 1) for i in range(len(names))]


def main():
    text = synth_text()
    with open(os.path.join(HERE, "synth_inject.gfa"), "wb") as f:
        f.write(text)
    manifest = {"synth_inject.gfa": {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "spec": SYNTH}, "left_out": {}}
    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))) + [os.path.join(HERE, "synth_inject.gfa")]:
        stem = os.path.basename(gfa)[:-4]
        with open(gfa, "rb") as f:
            src = f.read()
        if not named_in_order(src):
            manifest["left_out"][stem] = "segment names are not 1..S in file order: slow_odgi renumbers by numeric name"
            continue
        bed = slow_odgi(["inject_setup"], gfa)
        bed_path = os.path.join(HERE, stem + ".inject.bed")
        with open(bed_path, "wb") as f:
            f.write(bed)
        out = slow_odgi(["inject", "--bed", bed_path], gfa)
        with open(os.path.join(HERE, stem + ".inject.gfa"), "wb") as f:
            f.write(out)
        count = lambda t, c: sum(ln.startswith(c) for ln in t.split(b"\n"))  # noqa: E731
        cuts, added = count(out, b"S\t") - count(src, b"S\t"), count(out, b"P\t") - count(src, b"P\t")
        manifest[stem] = {"bed_sha256": hashlib.sha256(bed).hexdigest(), "bed_lines": bed.count(b"\n"),
                          "gfa_sha256": hashlib.sha256(out).hexdigest(), "gfa_bytes": len(out), "cuts": cuts, "paths_added": added,
                          "input_ends_in_newline": src.endswith(b"\n")}
        if cuts == 0:
            manifest[stem]["note"] = "the reference cut nothing here: this fixture checks the new paths only"
        print(stem, bed.count(b"\n"), cuts, added)
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
