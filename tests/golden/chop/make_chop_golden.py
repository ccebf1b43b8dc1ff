"""Regenerates the chop goldens: `slow_odgi chop GFA -n 3` (the reference's tests/turnt.toml chop_test) on every
tests/golden/*.gfa whose segments all have a sequence and distinct names -- slow_odgi gives an empty segment no piece and
keys segments by name, where chop.rs keeps one piece and every segment.  Needs the reference's slow_odgi and mygfa on
PYTHONPATH; the tests only read the outputs, <name>.chop3.gfa in this directory.

    PYTHONPATH=REFERENCE/slow_odgi:REFERENCE/mygfa python tests/golden/chop/make_chop_golden.py
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)


def eligible(path):
    names, empty = [], False
    with open(path, "rb") as f:
        for ln in f.read().split(b"\n"):
            fl = ln.split(b"\t")
            if fl[0] == b"S":
                names.append(fl[1])
                empty = empty or len(fl) < 3 or fl[2] in (b"", b"*")
    return names and not empty and len(set(names)) == len(names)


def main():
    for gfa in sorted(glob.glob(os.path.join(GOLDEN, "*.gfa"))):
        name = os.path.basename(gfa)[:-4]
        if not eligible(gfa):
            print("skip", name)
            continue
        out = subprocess.run([sys.executable, "-m", "slow_odgi", "chop", gfa, "-n", "3"], check=True, capture_output=True,
                             timeout=600).stdout
        with open(os.path.join(HERE, name + ".chop3.gfa"), "wb") as f:
            f.write(out)
        print("wrote", name, len(out))


if __name__ == "__main__":
    main()
