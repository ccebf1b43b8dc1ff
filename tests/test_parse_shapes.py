"""The plain grammar of the device GFA parser, restated in tests/parse_shapes.py, against the texts the suite has: every
golden GFA and every handmade text is plain (so the GPU tests may demand the device route for them), and of the parser
quirks exactly the listed ones are not.  The shapes' own assertions run for a tile of 4096 bytes.  No GPU needed."""
import numpy as np
import pytest

import pollen_amd as pa
import parse_shapes as ps
from test_host import QUIRKS


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("gfa", ps.all_golden_gfas(), ids=ps.golden_id)
def test_goldens_are_plain(gfa):
    text = read(gfa)
    assert ps.reason(text) == "plain" and ps.reason(text, True) == "plain"


def test_there_are_69_goldens_and_one_lacks_its_last_newline():
    texts = [read(g) for g in ps.all_golden_gfas()]
    assert len(texts) == 69
    assert [ps.golden_id(g) for g, t in zip(ps.all_golden_gfas(), texts) if not t.endswith(b"\n")] == ["ref_handmade_no-test-flip4"]


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade_texts_are_plain(name):
    assert ps.plain(ps.HANDMADE[name]) and ps.plain(ps.HANDMADE[name], True)


def test_quirks_the_grammar_excludes():
    assert len(QUIRKS) == 30
    got = {i: ps.reason(t) for i, t in enumerate(QUIRKS) if not ps.plain(t)}
    assert got == ps.QUIRKS_NOT_PLAIN
    assert {i: ps.reason(t) for i, t in enumerate(ps.ADDED) if not ps.plain(t)} == ps.ADDED_NOT_PLAIN


def test_plain_quirks_parse_on_the_host():
    """A plain text is one the host parser accepts: the device route never hides an error."""
    for t in QUIRKS + ps.ADDED:
        for stream in (False, True):
            if ps.plain(t, stream):
                (pa.parse_stream_bytes if stream else pa.parse_bytes)(t)


def test_stream_mode_sees_the_last_line():
    assert ps.plain(b"S\t1\tA\nX") and ps.reason(b"S\t1\tA\nX", True) == "grammar"
    assert ps.plain(b"S\t1\tA\nP\tp\t2+\t*") and ps.reason(b"S\t1\tA\nP\tp\t2+\t*", True) == "name"
    assert ps.lines_of(b"", True) == [] and ps.lines_of(b"S\t1\tA\n", True) == [b"S\t1\tA"]


def test_limits_and_precedence():
    long_name = b"0" * 32 + b"7"
    assert ps.reason(b"S\t" + long_name + b"\tA\n") == "limit"
    assert ps.plain(b"S\t" + long_name[1:] + b"\tA\n")                           # 32 digits are read
    assert ps.reason(b"S\t1\tA\nP\tp\t" + long_name + b"+\t*\n") == "limit"      # (before its name is looked up)
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t" + long_name + b"M\n") == "limit"
    assert ps.reason(b"S\t" + long_name + b"\tA\nX\n") == "grammar"              # grammar first
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t4294967297M\n") == "plain"        # parse_num::<u32> wraps to 1
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t256M\n") == "grammar"
    assert ps.reason(b"S\t0\tA\nP\tp\t0+\t*\n") == "name"                        # name 0 never resolves (namemap.rs:28)


def test_shapes_hold_for_a_4_kib_tile():
    T = 4096
    for k in range(-1, 8):
        assert ps.plain(ps.item_on_edge(T, k))
    for make in (ps.field_begins_on_tile, ps.field_ends_on_tile, ps.short_lines_in_one_tile, ps.line_across_tiles,
                 ps.newline_ends_tile, ps.newline_begins_tile):
        text = make(T)
        assert ps.plain(text) and ps.plain(text, True)
        pa.parse_bytes(text)
    for text in (ps.many_short_paths(), ps.reversed_names(), ps.skipped_names(), ps.duplicate_names(T, True),
                 ps.duplicate_names(T, False), ps.digit_names()):
        assert ps.plain(text)
        pa.parse_bytes(text)
    assert [len(ps.steps_exact(n)) for n in (5, 6, 7, 100)] == [5, 6, 7, 100]


def test_normalized_pools():
    """The identity, but for the line order, on a text in normalized order; an empty alignment becomes the printer's 0M."""
    for text in (ps.HANDMADE["only a header"], b"H\tVN:Z:1.0\nS\t1\tA\nS\t2\tC\nP\tp\t1+,2-\t2M,1M3D\nP\tq\t2+\t*\nL\t1\t+\t2\t-\t4M\nL\t2\t+\t1\t+\t0M\n"):
        with pa.parse_bytes(text) as g:
            want = ps.pools_of(g)
            want["line_order"] = b""
            assert ps.normalized_pools(g) == want
    # file order L, P: the link's ops move behind the path's; a link without ops gets one
    with pa.parse_bytes(b"S\t1\tA\nL\t1\t+\t1\t-\t\nL\t1\t-\t1\t+\t7M\nP\tp\t1+,1-\t2M\n") as g:
        assert (g.pool("alignment") >> 8).tolist() == [7, 2]
        n = ps.normalized_pools(g)
        assert np.frombuffer(n["alignment"], "<u4").tolist() == [2 << 8, 0, 7 << 8]
        assert np.frombuffer(n["links"], "<u4").reshape(-1, 4)[:, 2:].tolist() == [[1, 2], [2, 3]]
        assert np.frombuffer(n["overlaps"], "<u4").tolist() == [0, 1]
