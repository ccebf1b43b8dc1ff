"""The device GFA printer (`fgfa print`, FlatGFA.gfa_text_device / gfa_stream / gfa_bytes / write_gfa_device) against the
host printer (FlatGFA.gfa_text) and tests/print_model.py, byte for byte: every golden graph and the handmade texts, through
the buffer call, the stream, the file and the command line; resident handles; the graphs chop, inject, crush and extract
make, and their command-line forms, which print through the device.  Run with -m gpu."""
import os
import subprocess

import pytest

import pollen_amd as pa
import print_model as pm
import print_shapes as ps
from conftest import ROOT, fixture_id, golden_gfas
from pollen_amd import _lib
from test_print_model import load

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
ERR_IO = -5


def fgfa(*args, cwd=None):
    r = subprocess.run([FGFA, *args], capture_output=True, timeout=120, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r.stdout


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check_python(g, want, tmp_path):
    """Every Python route of one handle gives `want`."""
    got = g.gfa_text_device()
    assert len(got) == len(want) and got == want
    pieces = []
    g.gfa_stream(pieces.append)
    assert b"".join(pieces) == want and all(pieces)
    assert g.gfa_bytes() == len(want)
    out = str(tmp_path / "written.gfa")
    g.write_gfa_device(out)
    assert read(out) == want


def check_text(text, tmp_path):
    src = tmp_path / "in.gfa"
    src.write_bytes(text)
    with pa.parse_bytes(text) as g:
        want = g.gfa_text()
        assert want == pm.gfa(pm.pools_of(g))
        check_python(g, want, tmp_path)
        assert fgfa("-I", str(src), "print") == want
        g.write_flatgfa(str(tmp_path / "in.flatgfa"))
        assert fgfa("-i", str(tmp_path / "in.flatgfa"), "print", "-O", str(tmp_path / "cli.gfa")) == b""
        assert read(tmp_path / "cli.gfa") == want
        # resident: the steps are read in place
        g.to_device(0)
        check_python(g, want, tmp_path)


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_golden(gfa, tmp_path):
    check_text(read(gfa), tmp_path)


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade(name, tmp_path):
    check_text(ps.HANDMADE[name], tmp_path)


def test_o_before_the_command(tmp_path):
    src = tmp_path / "in.gfa"
    src.write_bytes(ps.HANDMADE["plain"])
    assert fgfa("-I", str(src), "-O", str(tmp_path / "o.gfa"), "print") == b""
    assert read(tmp_path / "o.gfa") == ps.HANDMADE["plain"]


def graph_text():
    """A graph with Ns to crush, paths to cut and links to follow."""
    out = [b"H\tVN:Z:1.0"]
    for i in range(1, 41):
        out.append(b"S\t%d\t%s" % (i, (ps.bases(3 + i % 9, i) + b"NNN" * (i % 3) + ps.bases(i % 4, i + 99))))
    out += [b"L\t%d\t+\t%d\t+\t0M" % (i, i + 1) for i in range(1, 40)]
    out.append(b"P\tx\t" + b",".join(b"%d+" % i for i in range(1, 41)) + b"\t*")
    out.append(b"P\ty\t" + b",".join(b"%d+" % i for i in range(5, 30)) + b"\t*")
    return b"\n".join(out) + b"\n"


BED = b"x\t7\t60\tleft\ny\t3\t41\tright\n"
MAKERS = {
    "chop": (lambda g: g.chop(3), ["chop", "-c", "3"]),
    "chop -l": (lambda g: g.chop(3, links=True), ["chop", "-c", "3", "-l"]),
    "crush": (lambda g: g.crush(), ["crush"]),
    "inject": (lambda g: g.inject(BED, links=True), ["inject", "-b", "BED", "-l"]),
    "extract": (lambda g: g.extract(12, 3), ["extract", "-n", "12", "-c", "3"]),
}


@pytest.mark.parametrize("what", list(MAKERS))
def test_outputs_of_the_other_features(what, tmp_path):
    make, args = MAKERS[what]
    text = graph_text()
    src, bed = tmp_path / "g.gfa", tmp_path / "in.bed"
    src.write_bytes(text)
    bed.write_bytes(BED)
    args = [str(bed) if a == "BED" else a for a in args]
    with pa.parse_bytes(text) as g, make(g) as q:
        assert len(q.pool("line_order")) == 0  # normalized order
        want = q.gfa_text()
        assert want == pm.gfa(pm.pools_of(q)) and len(want) > 100
        check_python(q, want, tmp_path)
        # the command prints through the device: the host printer's bytes of the same graph
        assert fgfa("-I", str(src), *args) == want
        assert fgfa("-I", str(src), "-O", str(tmp_path / "cli.gfa"), *args) == b""
        assert read(tmp_path / "cli.gfa") == want


def test_sink_stops_the_call():
    lib = _lib.lib()
    with pa.synth(3, 5_000, 4, 400_000) as g:  # more than two pieces of text
        want = g.gfa_text()
        assert len(want) > 2 * ps.PIECE
        calls = []

        def sink(_ctx, ptr, n):
            calls.append(n)
            return 7 if len(calls) == 2 else 0
        rc = lib.flatgfa_print_gfa_stream(g._h, _lib.SINK_T(sink), None)
        assert rc == ERR_IO and len(calls) == 2, (rc, calls)
        assert "sink" in _lib.last_error()
        # a writer that raises: the exception comes out, nothing more is written
        seen = []

        def boom(b):
            seen.append(len(b))
            raise OSError("disk full")
        with pytest.raises(OSError):
            g.gfa_stream(boom)
        assert len(seen) == 1
        assert g.gfa_text_device() == want  # the handle answers after a stopped call


def test_path_with_no_steps(tmp_path):
    p = ps.path_without_steps(ps.HANDMADE["path overlaps"], 1)
    with load(p, tmp_path) as g:
        calls = []
        with pytest.raises(pa.FlatGFAError) as e:
            g.gfa_stream(calls.append)
        assert e.value.code == -2 and _lib.last_error() == "print: path with no steps" and calls == []
    for extra in ([], ["-O", str(tmp_path / "out.gfa")]):
        r = subprocess.run([FGFA, "-i", str(tmp_path / "shape.flatgfa"), "print", *extra], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and b"print: path with no steps" in r.stderr
        assert not os.path.exists(tmp_path / "out.gfa")


def test_step_that_names_no_segment(tmp_path):
    with load(ps.bad_step(ps.HANDMADE["plain"]), tmp_path) as g:
        for call in (g.gfa_bytes, g.gfa_text_device, lambda: g.gfa_stream(lambda b: None)):
            with pytest.raises(pa.FlatGFAError) as e:
                call()
            assert e.value.code == -2 and "out of range" in _lib.last_error()


def test_empty_graph(tmp_path):
    with pa.parse_bytes(b"") as g:
        assert g.gfa_text() == b""
        calls = []
        g.gfa_stream(calls.append)
        assert calls == [] and g.gfa_bytes() == 0 and g.gfa_text_device() == b""
        g.write_gfa_device(str(tmp_path / "empty.gfa"))
        assert read(tmp_path / "empty.gfa") == b""
    src = tmp_path / "in.gfa"
    src.write_bytes(b"")
    assert fgfa("-I", str(src), "print") == b""
    assert fgfa("-I", str(src), "print", "-O", str(tmp_path / "cli.gfa")) == b"" and read(tmp_path / "cli.gfa") == b""


def test_pools_no_text_gives(tmp_path):
    text = ps.alternating(12)
    for p in (ps.short_line_order(text, 7), ps.normalized(text), ps.shared_steps(text), ps.normalized(ps.HANDMADE["P before S"]),
              ps.wide_ops(ps.long_cigar(30, 10)), ps.wide_ops(ps.HANDMADE["path overlaps"]), ps.normalized(ps.HANDMADE["only a header"])):
        with load(p, tmp_path) as g:
            want = g.gfa_text()
            assert want == pm.gfa(p)
            check_python(g, want, tmp_path)
