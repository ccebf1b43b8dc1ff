"""Every generator of tests/gaf_lookup_shapes.py, and every closed form the GPU suite uses at large size, against the model."""
import os

import gaf_lookup_model as M
import gaf_lookup_shapes as Sh
from conftest import GOLDEN, golden_gfas


def tiny():
    return M.Graph.from_gfa(open(os.path.join(GOLDEN, "ref_tiny.gfa"), "rb").read())


def test_random_reads_are_valid_on_every_golden_graph():
    seen_back = seen_none = 0
    for path in golden_gfas():
        g = M.Graph.from_gfa(open(path, "rb").read())
        if not g.names:
            continue
        text = Sh.random_reads(g, 5, 30)
        r = M.reads(g, text, want_bases=True)  # no error: names known, start <= end inside the walk
        assert len(r) == 30
        seen_back += sum(e[0] & 1 for _, evs in r for e in evs)
        seen_none += sum(e[1] == M.NONE for _, evs in r for e in evs)
        assert Sh.random_reads(g, 5, 30) == text  # seeded
    assert seen_back and seen_none


def test_padded_reads_cross_the_boundary_with_every_part():
    g = tiny()
    for boundary in (Sh.STEP, 256):
        text = Sh.padded_reads(g, 3, boundary, span=40)
        r = M.reads(g, text, want_bases=True)
        assert len(r) == 80
        # the filler read of variant k ends k bytes (mod boundary) short of a boundary
        off = 0
        for k in range(40):
            filler_end = text.index(b"\n", off) + 1
            assert (filler_end + k) % boundary == 0
            off = text.index(b"\n", filler_end) + 1


def test_long_path_line_closed_form():
    g = tiny()
    for n in (1, 7, 200):
        line = Sh.long_path_line(g, n, 3, 40)
        assert M.count(g, line) == (Sh.long_path_count(n), 1)


def test_many_short_lines_closed_form():
    g = tiny()
    text = Sh.many_short_lines(g.names[0], 50)
    assert M.seqs_text(g, text) == Sh.many_short_lines_seqs(g.seqs[0], 50)
    assert M.count(g, text) == (50, 50)


def test_big_segment_closed_form():
    for n in (10, 333):
        gfa, big = Sh.big_segment_gfa(n)
        g = M.Graph.from_gfa(gfa)
        assert [len(s) for s in g.seqs] == [5, n, 0]
        assert any(c in big for c in b"acgt") and (n < 100 or b"N" in big)
        assert M.seqs_text(g, Sh.big_segment_reads(n)) == Sh.big_segment_seqs(big)


def test_zero_byte_events():
    g = tiny()
    line = Sh.zero_byte_events(g.names, 300)
    (name, evs), = M.reads(g, line, want_bases=True)
    assert len(evs) == 301 and all(e[1] == M.NONE for e in evs[1:])
    assert M.seqs_text(g, line) == b"z\t" + g.seqs[0][:1] + b"\n"


def test_bad_lines_give_their_codes():
    g = tiny()
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    for name, (line, code) in Sh.BAD_LINES.items():
        try:
            M.reads(g, ok + line + b"\n" + ok)
            assert False, name
        except M.LookupError_ as e:
            assert (e.code, e.offset) == (code, len(ok)), name
