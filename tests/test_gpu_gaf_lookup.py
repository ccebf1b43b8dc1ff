"""The GAF lookup on the GPU (`fgfa gaf`, flatgfa_gaf_*, FlatGFA.all_reads) against tests/gaf_lookup_model.py."""
import ctypes
import os
import subprocess

import pytest

import gaf_lookup_model as M
import gaf_lookup_shapes as Sh
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas

pytestmark = pytest.mark.gpu

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
TINY_GFA = os.path.join(GOLDEN, "ref_tiny.gfa")
TINY_GAF = os.path.join(GOLDEN, "gaf", "tiny.gaf")
ERR_BOUNDS, ERR_PARSE = -2, -7


def load(path):
    import pollen_amd as pa
    text = open(path, "rb").read()
    return pa.parse_bytes(text), M.Graph.from_gfa(text)


def fgfa(*args):
    return subprocess.run([FGFA, "-I", TINY_GFA, "gaf"] + list(args), capture_output=True, timeout=120)


def test_known_answers_python():
    # flatgfa-py/test/test_gaf.py, as it is written there
    g, _ = load(TINY_GFA)
    gaf = g.all_reads(TINY_GAF)
    assert ["".join(e.sequence() for e in line) for line in gaf] == ["AAGAAATTTTCT", "GAAATTTTCTGGAGTTCTAT"]
    assert [[e.range for e in line] for line in gaf] == [[(5, 8), (0, 9), (1, 0)], [(7, 8), (0, 18), (0, 0)]]
    assert [line.name for line in gaf] == ["foo", "bar"]
    assert [line.sequence() for line in gaf] == ["AAGAAATTTTCT", "GAAATTTTCTGGAGTTCTAT"]
    assert gaf[0].segment_ranges() == "\n0: 1+, 5-8bp\n1: 2+, 0-9bp\n2: (skipped)"
    assert [str(e.handle) for e in gaf[0].chunks] == ["1+", "2+", "4-"]
    assert g.gaf_count(TINY_GAF) == 6
    assert g.gaf_seqs(open(TINY_GAF, "rb").read()) == b"foo\tAAGAAATTTTCT\nbar\tGAAATTTTCTGGAGTTCTAT\n"


def test_known_answers_cli_and_print(capfdbinary):
    want_s = b"foo\tAAGAAATTTTCT\nbar\tGAAATTTTCTGGAGTTCTAT\n"
    r = fgfa(TINY_GAF, "-s")
    assert (r.returncode, r.stdout) == (0, want_s)
    r = fgfa(TINY_GAF)
    assert (r.returncode, r.stdout) == (0, b"foo\n0: 1+, 5-8bp1: 2+, 0-9bp2: (skipped)bar\n0: 1+, 7-8bp1: 2+, 19bp2: 3+, 0-0bp")
    for flags in (["-b"], ["-b", "-p"], ["-p", "-b"]):
        r = fgfa(TINY_GAF, *flags)
        assert (r.returncode, r.stdout) == (0, b"6\n"), flags
    g, _ = load(TINY_GFA)
    capfdbinary.readouterr()
    g.print_gaf_lookup(TINY_GAF)
    assert capfdbinary.readouterr().out == want_s


def test_cli_usage_and_unreadable_file():
    for args in ([TINY_GAF, "-p"], [], [TINY_GAF, "extra.gaf"], [TINY_GAF, "-x"], ["-s"]):
        r = fgfa(*args)
        assert r.returncode == 2 and r.stdout == b"" and b"usage" in r.stderr, args
    r = fgfa(os.path.join(GOLDEN, "gaf", "no_such.gaf"), "-s")
    assert r.returncode == 1 and r.stdout == b""


def test_known_answers_c_abi():
    from pollen_amd import _lib
    from pollen_amd.gaf import flatgfa_gaf_events_t
    g, _ = load(TINY_GFA)
    text = open(TINY_GAF, "rb").read()
    lib = _lib.lib()
    ev, ln = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.flatgfa_gaf_count(g._h, text, len(text), ctypes.byref(ev), ctypes.byref(ln)) == 0
    assert (ev.value, ln.value) == (6, 2)
    out = ctypes.POINTER(flatgfa_gaf_events_t)()
    assert lib.flatgfa_gaf_events(g._h, text, len(text), ctypes.byref(out)) == 0
    e = out.contents
    u64 = lambda p, n: list((ctypes.c_uint64 * n).from_address(p))  # noqa: E731
    assert (e.n_lines, e.n_events) == (2, 6)
    assert u64(e.line_first, 3) == [0, 3, 6]
    assert u64(e.name_off, 2) == [0, text.index(b"\n") + 1] and u64(e.name_len, 2) == [3, 3]
    assert list((ctypes.c_uint32 * 6).from_address(e.handle)) == [0, 2, 7, 0, 2, 4]
    assert list((ctypes.c_uint8 * 6).from_address(e.kind)) == [2, 2, 0, 2, 1, 2]
    assert u64(e.a, 6) == [5, 0, 0, 7, 0, 0] and u64(e.b, 6) == [8, 9, 0, 8, 19, 0]
    lib.flatgfa_gaf_events_free(out)
    # no text: no lines, no error
    assert lib.flatgfa_gaf_count(g._h, None, 0, ctypes.byref(ev), ctypes.byref(ln)) == 0 and (ev.value, ln.value) == (0, 0)
    assert g.gaf_seqs(b"") == b"" and g.gaf_table(b"no newline") == b"" and len(g.all_reads(b"")) == 0


@pytest.mark.parametrize("path", golden_gfas(), ids=fixture_id)
def test_random_walks_on_every_golden_graph(path):
    g, mg = load(path)
    text = Sh.random_reads(mg, 11, 200) if mg.names else b""  # (a graph without segments has no walks)
    assert g.gaf_seqs(text) == M.seqs_text(mg, text)
    assert g.gaf_table(text) == M.table_text(mg, text)
    assert g.gaf_count(text) == M.count(mg, text)[0]
    want = M.reads(mg, text)
    got = g.all_reads(text)
    assert len(got) == len(want)
    for line, (name, evs) in zip(got, want):
        assert line.name.encode() == name
        assert [(e.handle._bits, e.range) for e in line] == [(ev[0], M.py_range(mg, ev)) for ev in evs]
        assert line.sequence().encode("latin-1") == b"".join(M.event_bases(mg, ev) for ev in evs)


@pytest.mark.parametrize("name", sorted(Sh.BAD_LINES))
def test_each_error_kind(name, tmp_path):
    import pollen_amd as pa
    g, mg = load(TINY_GFA)
    line, code = Sh.BAD_LINES[name]
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    text = ok * 3 + line + b"\n" + ok
    want = ERR_PARSE if code == "parse" else ERR_BOUNDS
    for call in (g.gaf_seqs, g.gaf_table, g.gaf_count, g.all_reads):
        with pytest.raises(pa.FlatGFAError) as ei:
            call(text)
        assert ei.value.code == want, (name, call)
        assert f"byte offset {3 * len(ok)} " in str(ei.value), str(ei.value)
    f = tmp_path / "bad.gaf"
    f.write_bytes(text)
    for flags in ([], ["-s"], ["-b"]):
        r = fgfa(str(f), *flags)
        assert r.returncode == 1 and r.stdout == b"" and str(3 * len(ok)).encode() in r.stderr, (name, flags)


def test_end_below_start_is_an_error_only_for_bases():
    import pollen_amd as pa
    g, mg = load(TINY_GFA)
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    text = ok + Sh.gaf_line(b"r", b">1>2", 6, 2) + Sh.gaf_line(b"w", b">1>2", 9, 3) + ok
    assert g.gaf_table(text) == M.table_text(mg, text)  # the wrapped numbers print as the reference's would
    assert g.gaf_count(text) == 6
    reads = g.all_reads(text)
    assert reads[1].chunks[0].range == (6, 2) and reads[2].chunks[1].range == (1, (3 - 8) & M.U64)
    with pytest.raises(IndexError):
        reads[1].sequence()
    with pytest.raises(pa.FlatGFAError) as ei:
        g.gaf_seqs(text)
    assert ei.value.code == ERR_BOUNDS and f"byte offset {len(ok)} " in str(ei.value)


def test_lowest_offset_decides_between_kinds(monkeypatch):
    import pollen_amd as pa
    g, _ = load(TINY_GFA)
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    bad_name = Sh.BAD_LINES["unknown_name"][0] + b"\n"
    bad_parse = Sh.BAD_LINES["eight_tabs"][0] + b"\n"
    bad_slice = Sh.gaf_line(b"r", b">1", 6, 2)
    for chunk in (None, "1"):  # one chunk; a chunk per line
        if chunk:
            monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
        for first, second, code in ((bad_name, bad_parse, ERR_BOUNDS), (bad_parse, bad_name, ERR_PARSE), (bad_slice, bad_parse, ERR_BOUNDS),
                                    (bad_parse, bad_slice, ERR_PARSE)):
            with pytest.raises(pa.FlatGFAError) as ei:
                g.gaf_seqs(ok * 2 + first + ok + second)
            assert ei.value.code == code and f"byte offset {2 * len(ok)} " in str(ei.value)


def test_graph_that_is_not_resident_stays_so():
    g, mg = load(TINY_GFA)
    lib = __import__("pollen_amd")._lib.lib()
    h2d, plan = ctypes.c_double(), ctypes.c_double()
    assert lib.flatgfa_residency_ms(g._h, ctypes.byref(h2d), ctypes.byref(plan)) != 0
    text = open(TINY_GAF, "rb").read()
    assert g.gaf_seqs(text) == M.seqs_text(mg, text) and g.gaf_count(text) == 6 and len(g.all_reads(text)) == 2
    assert lib.flatgfa_residency_ms(g._h, ctypes.byref(h2d), ctypes.byref(plan)) != 0  # still not resident
    d, _u = g.seg_depth_with_uniq()  # and a resident graph answers the same
    assert list(d) == [2, 2, 1, 2]
    assert g.gaf_seqs(text) == M.seqs_text(mg, text)


def test_token_stop_rule():
    # gaf.rs:287-308: the walk stops silently at the first byte that continues no token; the matrix would count every '>'
    g, mg = load(TINY_GFA)
    paths = [b">1x>2", b">1><2", b"1>2", b"", b">1>2>", b">1>2<x4", b">1 >2", b">999999"[:1] + b"1>2y>999999"]
    text = b"".join(Sh.gaf_line(b"t%d" % i, p, 2, 12) for i, p in enumerate(paths))
    assert [len(evs) for _, evs in M.reads(mg, text)] == [1, 1, 0, 0, 2, 2, 1, 2]
    assert g.gaf_seqs(text) == M.seqs_text(mg, text)
    assert g.gaf_table(text) == M.table_text(mg, text)
    assert g.gaf_count(text) == 9
    assert [len(r) for r in g.all_reads(text)] == [1, 1, 0, 0, 2, 2, 1, 2]
