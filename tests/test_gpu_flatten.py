"""The GPU flatten (`fgfa flatten`, FlatGFA.flatten_*) against the reference's own bytes (tests/golden/flatten, written by
`slow_odgi flatten`) where the input ends in a newline, and against tests/flatten_model.py always: through the buffer calls,
the stream, the files and the command line.  Run with -m gpu."""
import ctypes
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

import chop_model as cm
import flatten_model as fm
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from test_flatten_model import CASES, FLAT, MANIFEST

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
ERR_IO = -5
IDS = [s for s, _ in CASES]


def fgfa(*args, cwd=None):
    r = subprocess.run([FGFA, *args], capture_output=True, timeout=120, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r.stdout


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("stem,gfa", CASES, ids=IDS)
def test_golden_python(stem, gfa):
    name = stem.encode() + b".og"
    text = read(gfa)
    p = fo.parse_gfa(text)
    with pa.parse_bytes(text) as g:
        fasta, bed = g.flatten_fasta(name), g.flatten_bed(name)
        assert fasta == fm.fasta(p, name) and bed == fm.bed(p, name)
        if MANIFEST[stem + ".flatten.txt"]["input_ends_in_newline"]:
            assert fasta + bed == read(os.path.join(FLAT, stem + ".flatten.txt"))
        assert g.flatten_legend().tolist() == fm.legend(p)
        f, b = io.BytesIO(), io.BytesIO()
        g.flatten_to(name, f, b)
        assert f.getvalue() == fasta and b.getvalue() == bed
        pieces = []
        g.flatten_stream(name, 3, pieces.append)
        assert b"".join(pieces) == fasta + bed
        # resident: the steps are read in place
        g.to_device(0)
        assert g.flatten_bed(b"other") == fm.bed(p, b"other") and g.flatten_fasta(b"") == fm.fasta(p, b"")


@pytest.mark.parametrize("stem,gfa", CASES, ids=IDS)
def test_golden_cli(stem, gfa, tmp_path):
    text = read(gfa)
    p = fo.parse_gfa(text)
    want = fm.flatten(p, stem.encode() + b".og")
    if MANIFEST[stem + ".flatten.txt"]["input_ends_in_newline"]:
        assert want == read(os.path.join(FLAT, stem + ".flatten.txt"))
    # -I, to stdout, the default NAME: from inside the directory, as the golden was made
    assert fgfa("-I", os.path.basename(gfa), "flatten", cwd=os.path.dirname(gfa)) == want
    # -i, to files, with -n
    with pa.parse_bytes(text) as g:
        g.write_flatgfa(str(tmp_path / (stem + ".flatgfa")))
    assert fgfa("-i", stem + ".flatgfa", "flatten", "-n", "chr@1", "-f", "out.fa", "-b", "out.bed", cwd=tmp_path) == b""
    assert read(tmp_path / "out.fa") == fm.fasta(p, b"chr@1") and read(tmp_path / "out.bed") == fm.bed(p, b"chr@1")


def test_cli_the_other_ways(tmp_path):
    stem, gfa = next(c for c in CASES if c[0] == "synth_flat")
    text = read(gfa)
    p = fo.parse_gfa(text)
    with pa.parse_bytes(text) as g:
        g.write_flatgfa(str(tmp_path / "some.dir.flatgfa"))
    # -i, to stdout, the default NAME: the last extension cut
    assert fgfa("-i", "some.dir.flatgfa", "flatten", cwd=tmp_path) == fm.flatten(p, b"some.dir.og")
    assert fgfa("-i", "some.dir.flatgfa", "flatten", "-n", "", cwd=tmp_path) == fm.flatten(p, b"")
    # -I, one file only: nothing on stdout, the other text nowhere
    assert fgfa("-I", gfa, "flatten", "-b", str(tmp_path / "only.bed")) == b""
    assert read(tmp_path / "only.bed") == fm.bed(p, gfa[:-4].encode() + b".og")
    assert fgfa("-I", gfa, "flatten", "-n", "n", "-f", str(tmp_path / "only.fa")) == b""
    assert read(tmp_path / "only.fa") == fm.fasta(p, b"n") and not os.path.exists(tmp_path / "out.bed")
    # usage errors: 2, nothing printed
    for bad in (["flatten", "-x"], ["flatten", "-n"], ["flatten", "extra"]):
        r = subprocess.run([FGFA, "-I", gfa, *bad], capture_output=True, timeout=120)
        assert r.returncode == 2 and r.stdout == b"" and b"usage: fgfa flatten" in r.stderr


def test_sink_stops_the_call():
    lib = _lib.lib()
    _, gfa = next(c for c in CASES if c[0] == "synth_flat")
    with pa.parse_bytes(read(gfa)) as g:
        for what in (1, 2, 3):
            calls = []

            def sink(_ctx, ptr, n, calls=calls):
                calls.append(n)
                return 7 if len(calls) == 2 else 0
            rc = lib.flatgfa_flatten_stream(g._h, b"x", 1, what, _lib.SINK_T(sink), None)
            assert rc == ERR_IO and len(calls) == 2, (what, rc, calls)
            assert "sink" in _lib.last_error()
        # a writer that raises: the exception comes out, nothing more is written
        seen = []

        def boom(b):
            seen.append(len(b))
            raise OSError("disk full")
        with pytest.raises(OSError):
            g.flatten_stream(b"x", 3, boom)
        assert len(seen) == 1
        assert g.flatten_bed(b"x") == fm.bed(fo.parse_gfa(read(gfa)), b"x")  # the handle answers after a stopped call


def test_chop_and_extract_outputs():
    """Their sequence spans are not in pool order: the FASTA is a gather."""
    _, gfa = next(c for c in CASES if c[0] == "synth_flat")
    with pa.parse_bytes(read(gfa)) as g:
        for make in (lambda: g.chop(3), lambda: g.chop(3, links=True), lambda: g.extract(5, 3)):
            with make() as q:
                p = cm.pools_of(q)
                assert q.flatten_fasta(b"q.og") == fm.fasta(p, b"q.og")
                assert q.flatten_bed(b"q.og") == fm.bed(p, b"q.og")
                assert q.flatten_legend().tolist() == fm.legend(p)
    text = read(os.path.join(os.path.dirname(FLAT), "ref_handmade_crush1.gfa"))
    with pa.parse_bytes(text) as g, g.extract(int(cm.pools_of(g).segs["name"][2]), 2) as q:
        p = cm.pools_of(q)
        starts = p.segs["seq_start"].astype(np.int64)
        assert len(starts) > 1
        assert q.flatten_fasta(b"e") + q.flatten_bed(b"e") == fm.flatten(p, b"e")


def test_mid_size_synthetic():
    with pa.synth(5, 20_000, 20, 10_000, with_seq=True) as g:
        p = cm.pools_of(g)
        assert len(p.steps) == 200_000
        want_f, want_b = fm.fasta(p, b"synth.og"), fm.bed_fast(p, b"synth.og")
        assert len(want_b) > fm.PIECE  # more than one piece
        got_f, got_b = g.flatten_fasta(b"synth.og"), g.flatten_bed(b"synth.og")
        assert len(got_f) == len(want_f) and hashlib.sha256(got_f).digest() == hashlib.sha256(want_f).digest()
        assert len(got_b) == len(want_b) and hashlib.sha256(got_b).digest() == hashlib.sha256(want_b).digest()
        h = hashlib.sha256()
        g.flatten_stream(b"synth.og", 3, h.update)
        assert h.digest() == hashlib.sha256(want_f + want_b).digest()
