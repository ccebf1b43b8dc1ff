"""tests/gaf_lookup_model.py against the reference's known answers and its own rules (no GPU)."""
import os

import gaf_lookup_model as M
import gaf_lookup_shapes as Sh
from conftest import GOLDEN


def tiny():
    g = M.Graph.from_gfa(open(os.path.join(GOLDEN, "ref_tiny.gfa"), "rb").read())
    return g, open(os.path.join(GOLDEN, "gaf", "tiny.gaf"), "rb").read()


def test_known_answers_of_the_reference():
    # flatgfa-py/test/test_gaf.py
    g, gaf = tiny()
    r = M.reads(g, gaf)
    assert [b"".join(M.event_bases(g, e) for e in evs) for _, evs in r] == [b"AAGAAATTTTCT", b"GAAATTTTCTGGAGTTCTAT"]
    assert [[M.py_range(g, e) for e in evs] for _, evs in r] == [[(5, 8), (0, 9), (1, 0)], [(7, 8), (0, 18), (0, 0)]]
    assert M.seqs_text(g, gaf) == b"foo\tAAGAAATTTTCT\nbar\tGAAATTTTCTGGAGTTCTAT\n"
    assert M.count(g, gaf) == (6, 2)


def test_default_listing_runs_together_byte_for_byte():
    # worked by hand from gaf.rs:167-197 and cmds.rs:367-374: no separator after an event, the next name follows directly;
    # line 2 ends exactly on segment 2's end, so its last token is Partial(0, 0)
    g, gaf = tiny()
    assert M.table_text(g, gaf) == b"foo\n0: 1+, 5-8bp1: 2+, 0-9bp2: (skipped)bar\n0: 1+, 7-8bp1: 2+, 19bp2: 3+, 0-0bp"
    assert M.table_text(g, b"q\t1\t0\t1\t+\t<4>1\t8\t0\t11\t1\t1\t0\n") == b"q\n0: 4-, 0-11bp1: 1+, 0-0bp"


def test_lines_are_the_bytes_before_a_newline_and_none_is_skipped():
    assert M.lines(b"a\n\n#c\ntail") == [(0, b"a"), (2, b""), (3, b"#c")]
    assert M.lines(b"no newline") == [] and M.lines(b"") == []
    g, _ = tiny()
    hash_line = b"#x\t1\t0\t1\t+\t>1\t8\t0\t1\t1\t1\t0\n"  # a '#' line is a read like any other
    assert M.seqs_text(g, hash_line) == b"#x\tC\n"


def test_closed_accept_rule_is_the_step_by_step_parser():
    n = 0
    for tabs in range(0, 13):
        for seed in range(3):
            for line in Sh.lines_with_tabs(tabs, seed):
                try:
                    M.parse_line(line)
                    ok = True
                except M.ParsePanic:
                    ok = False
                assert ok == M.accepts(line), line
                n += ok
    assert n > 50  # (the generator reaches the accepting side too)
    for name, (line, code) in Sh.BAD_LINES.items():
        assert M.accepts(line) == (code != "parse"), name
    assert not M.accepts(b"")
    name, start, end, path = M.parse_line(b"n\t1\t2\t3\t4\t>1\t6\t18446744073709551617\t007\t")
    assert (name, start, end, path) == (b"n", 1, 7, b">1")  # wrapping u64; the end's tab may be the line's last byte


def test_token_stop_rule():
    assert M.tokens(b">12x>13") == [(12, True)]
    assert M.tokens(b">1><2") == [(1, True)]
    assert M.tokens(b"12>3") == [] and M.tokens(b"") == [] and M.tokens(b">") == []
    assert M.tokens(b">12<34>5 suffix") == [(12, True), (34, False), (5, True)]  # gaf.rs:310-317
    assert M.tokens(b"<18446744073709551617") == [(1, False)]


def test_reverse_complement():
    assert M.revcomp(b"ACGTacgtNn-") == b"-nNacgtACGT"
    g = M.Graph([1], [b"AAcgN"])
    assert M.event_bases(g, (1, M.PARTIAL, 1, 4)) == M.revcomp(b"AAcgN")[1:4] == b"cgT"
    assert M.event_bases(g, (0, M.PARTIAL, 1, 4)) == b"Acg"
    assert M.event_bases(g, (1, M.ALL, 0, 5)) == b"NcgTT"
    assert M.event_bases(g, (0, M.PARTIAL, 3, 2)) is None and M.event_bases(g, (0, M.PARTIAL, 0, 6)) is None


def test_each_row_of_the_event_table():
    g = M.Graph([1, 2, 3, 4], [b"AAAA", b"", b"CCCCCC", b"GG"])  # lengths 4, 0, 6, 2
    walk = [(1, True), (2, True), (3, True), (4, True)]
    kinds = lambda s, e: [ev[1:] for ev in M.events(g, s, e, walk)]  # noqa: E731
    P, A, N = M.PARTIAL, M.ALL, M.NONE
    # starts and ends in the first token (row 1); everything behind it is None
    assert kinds(1, 3) == [(P, 1, 3), (N, 0, 0), (N, 0, 0), (N, 0, 0)]
    # starts in the first (row 2), the zero-length segment is All, ends in the third (row 3)
    assert kinds(1, 7) == [(P, 1, 4), (A, 0, 0), (P, 0, 3), (N, 0, 0)]
    # end == next of the first token: both compares are strict, so it does not end there; the empty segment is All and the next
    # token gets Partial(0, 0)
    assert kinds(0, 4) == [(P, 0, 4), (A, 0, 0), (P, 0, 0), (N, 0, 0)]
    # start == next of the first token: not started there, nor in the empty segment (start < next is false), but in the third
    assert kinds(4, 12) == [(N, 0, 0), (N, 0, 0), (P, 0, 6), (A, 0, 2)]
    # never started; never ended
    assert kinds(12, 13) == [(N, 0, 0)] * 4
    assert kinds(0, 99) == [(P, 0, 4), (A, 0, 0), (A, 0, 6), (A, 0, 2)]
    # an end below the start: a > b in the first row -- printed as it is, an error only where bases are asked for
    assert kinds(3, 1) == [(P, 3, 1), (N, 0, 0), (N, 0, 0), (N, 0, 0)]
    assert kinds(5, 2) == [(N, 0, 0), (N, 0, 0), (P, 1, (2 - 4) & M.U64), (N, 0, 0)]
    line = Sh.gaf_line(b"r", b">1>2>3>4", 3, 1)
    assert M.table_text(g, line) == b"r\n0: 1+, 3-1bp1: (skipped)2: (skipped)3: (skipped)"
    ok = b"ok\t1\t0\t1\t+\t>1\t8\t0\t1\t1\t1\t0\n"
    try:
        M.seqs_text(g, ok + line)
        assert False
    except M.LookupError_ as e:
        assert (e.code, e.offset) == ("bounds", len(ok))
    assert M.events(g, 0, 1, [(9, True)]) is None and M.events(g, 0, 1, [(0, True)]) is None


def test_lowest_offset_decides():
    g, _ = tiny()
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    bad_name = Sh.BAD_LINES["unknown_name"][0] + b"\n"
    bad_parse = Sh.BAD_LINES["eight_tabs"][0] + b"\n"
    for first, second, code in ((bad_name, bad_parse, "bounds"), (bad_parse, bad_name, "parse")):
        try:
            M.reads(g, ok + first + ok + second)
            assert False
        except M.LookupError_ as e:
            assert (e.code, e.offset) == (code, len(ok))
