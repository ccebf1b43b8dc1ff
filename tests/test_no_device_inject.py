"""What inject says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only route says.
Skipped where a device is visible.  The three refusals, the BED parse errors and the argument errors are decided before any
device work, so they are answered the same with and without a device, and are tested here."""
import ctypes
import os
import subprocess

import pytest

import pollen_amd as pa
from conftest import ROOT
from pollen_amd import _lib

TEXT = b"S\t1\tAAAA\nS\t2\tCC\nS\t3\tGGG\nP\tp\t1+,2-,3+\t*\nP\tq\t3-,1+\t*\nL\t1\t+\t2\t-\t0M\n"
MESSAGE = "no HIP device is visible; inject has no CPU fallback"
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")

ROUTES = {
    "bed text": lambda g: g.inject(b"p\t1\t5\tx\n"),
    "bed text, links": lambda g: g.inject(b"p\t1\t5\tx\n", links=True),
    "list": lambda g: g.inject([("p", 1, 5, "x"), (1, 0, 2, b"y")]),
    "no lines": lambda g: g.inject(b""),
    "only skipped lines": lambda g: g.inject(b"nope\t1\t5\tx\n"),
}


@pytest.mark.parametrize("what", list(ROUTES))
def test_no_device_message(what):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            ROUTES[what](g)
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == MESSAGE
    finally:
        g.close()


def test_cli_without_a_device(tmp_path):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    gfa, bed = tmp_path / "g.gfa", tmp_path / "b.bed"
    gfa.write_bytes(TEXT)
    bed.write_bytes(b"p\t1\t5\tx\n")
    r = subprocess.run([FGFA, "-I", str(gfa), "inject", "-b", str(bed)], capture_output=True, timeout=120)
    assert r.returncode == 1 and MESSAGE.encode() in r.stderr and r.stdout == b""


REFUSED = {
    "a new name is a path of the graph": (b"p\t1\t5\tq\n", "line 1"),
    "a new name twice": (b"p\t1\t5\tx\nq\t0\t3\tx\n", "line 2"),
    "a line on an injected path": (b"p\t4\t9\tx\nx\t1\t2\ty\n", "line 2"),
    "a new name twice, behind a comment and a skipped line": (b"# header\nnope\t1\t2\tz\np\t1\t5\tx\nq\t0\t3\tx\n", "line 4:"),
    "a path's name, behind a comment and an empty line": (b"# h\n\np\t1\t5\tq\n", "line 3:"),
    "an injected path, behind comments, skipped and empty lines": (b"#\nzz\t1\t2\ty\np\t1\t2\tx\n\nx\t1\t2\tw\n", "line 5 "),
    "a parse error behind a comment and an empty line": (b"# h\n\np\t1\t5\tx\np\t1\n", "line 4:"),
    "an empty new name": (b"p\t1\t5\tx\np\t1\t5\t\n", "line 2:"),
    "three columns": (b"p\t1\t5\tx\np\t1\t5\n", "line 2"),
    "no number": (b"# c\np\tone\t5\tx\n", "line 2"),
    "a number with a tail": (b"p\t1\t5x\tx\n", "line 1"),
    "one column": (b"p\n", "line 1"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_and_parse_errors_need_no_device(what):
    bed, where = REFUSED[what]
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            g.inject(bed)
        assert e.value.code == -1  # FLATGFA_ERR_ARG
        assert where in _lib.last_error() and "inject" in _lib.last_error()
    finally:
        g.close()


def test_a_repeated_name_behind_65536_lines_is_named_by_its_line_in_the_text():
    # more lines than 16 bits count, comments and empty lines among them: the refusal counts lines as the text has them
    rows, names = [], 0
    for i in range(66000):
        if i % 1000 == 7:
            rows.append(b"# a comment")
        elif i % 777 == 5:
            rows.append(b"")
        elif i % 501 == 3:
            rows.append(b"nope\t1\t2\tskipped%d" % i)
        else:
            rows.append(b"%s\t1\t5\tx%d" % (b"pq"[i % 2:i % 2 + 1], names))
            names += 1
    rows.append(b"q\t0\t3\tx40000")
    assert names > 65536 and len(rows) == 66001
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            g.inject(b"\n".join(rows) + b"\n")
        assert e.value.code == -1
        assert _lib.last_error() == "inject: line 66001: the new name was given by an earlier line"
        # and the same lines as a list, which has no text to count in: the line's index, from 1
        lines = [(f[0].decode(), int(f[1]), int(f[2]), f[3]) for f in (r.split(b"\t") for r in rows) if len(f) == 4 and f[0] != b"nope"]
        with pytest.raises(pa.FlatGFAError) as e:
            g.inject(lines)
        assert e.value.code == -1 and _lib.last_error() == "inject: line %d: the new name was given by an earlier line" % len(lines)
    finally:
        g.close()


def test_list_refusals_and_argument_errors_need_no_device():
    lib = _lib.lib()
    g = pa.parse_bytes(TEXT)
    out = ctypes.c_void_p()
    try:
        for lines in ([("p", 1, 5, "q")], [("p", 1, 5, "x"), ("q", 0, 3, "x")], [("p", 1, 5, "x"), ("q", 0, 3, "")]):
            with pytest.raises(pa.FlatGFAError) as e:
                g.inject(lines)
            assert e.value.code == -1
        with pytest.raises(KeyError):
            g.inject([("nope", 1, 5, "x")])
        assert lib.flatgfa_inject_bed(None, b"", 0, 0, ctypes.byref(out)) == -1
        assert lib.flatgfa_inject_bed(g._h, None, 3, 0, ctypes.byref(out)) == -1
        assert lib.flatgfa_inject_bed(g._h, b"", 0, 0, None) == -1
        assert lib.flatgfa_inject(g._h, None, None, None, None, None, 1, 0, ctypes.byref(out)) == -1
        assert lib.flatgfa_inject(None, None, None, None, None, None, 0, 0, ctypes.byref(out)) == -1
        n = ctypes.c_uint64()
        job = ctypes.c_void_p()
        assert lib.flatgfa_dev_inject_count(None, None, None, None, 0, None, None, ctypes.byref(job), ctypes.byref(n), ctypes.byref(n),
                                            ctypes.byref(n)) == -1
        graph = _lib.flatgfa_dev_graph_t()  # (no seg_len)
        assert lib.flatgfa_dev_inject_count(ctypes.byref(graph), None, None, None, 0, None, None, ctypes.byref(job), ctypes.byref(n),
                                            ctypes.byref(n), ctypes.byref(n)) == -1
        assert "seg_len" in _lib.last_error()
        assert lib.flatgfa_dev_inject_fill(None, None, None, None, None, None) == -1
        lib.flatgfa_dev_inject_free(None)
    finally:
        g.close()


def test_cli_usage_errors_exit_2(tmp_path):
    gfa = tmp_path / "g.gfa"
    gfa.write_bytes(TEXT)
    for args in (["inject"], ["inject", "-b"], ["inject", "-x", "y"], ["inject", "-l"]):
        r = subprocess.run([FGFA, "-I", str(gfa)] + args, capture_output=True, timeout=120, env=dict(os.environ, FLATGFA_NO_WARM="1"))
        assert r.returncode == 2 and b"usage: fgfa inject -b BED [-l]" in r.stderr, args
