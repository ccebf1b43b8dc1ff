"""tests/print_model.py, the restatement of print.rs that the device printer's tests compare with, equals the host printer
(FlatGFA.gfa_text) on every golden graph and on handmade texts that use each of its rules.  No GPU."""
import re

import pytest

import pollen_amd as pa
import print_model as pm
import print_shapes as ps
from conftest import fixture_id, golden_gfas


def read(path):
    with open(path, "rb") as f:
        return f.read()


def load(p, tmp_path):
    f = tmp_path / "shape.flatgfa"
    f.write_bytes(ps.fo.dump_flatgfa(p))
    return pa.load(str(f))


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_golden(gfa):
    with pa.parse_bytes(read(gfa)) as g:
        assert pm.gfa(pm.pools_of(g)) == g.gfa_text()


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade(name):
    text = ps.HANDMADE[name]
    with pa.parse_bytes(text) as g:
        got = pm.gfa(pm.pools_of(g))
        assert got == g.gfa_text()
        if text.endswith(b"\n") and name not in ("CIGARs of several ops", "path overlaps"):
            assert got == text  # the printer gives these texts back as they are (but D and I change places: print.rs:18-19)


def test_handmade_texts_use_the_rules():
    with pa.parse_bytes(ps.HANDMADE["header in the middle"]) as g:
        assert g.pool("line_order").tolist() == [pm.S, pm.S, pm.H, pm.L, pm.P]
    with pa.parse_bytes(ps.HANDMADE["P before S"]) as g:
        assert g.pool("line_order").tolist()[0] == pm.P
    with pa.parse_bytes(ps.HANDMADE["CIGARs of several ops"]) as g:
        assert len(g.pool("alignment")) == 4 + 1 + 2
    with pa.parse_bytes(ps.HANDMADE["path overlaps"]) as g:
        assert len(g.pool("overlaps")) == 3
    with pa.parse_bytes(ps.HANDMADE["a 20-digit name"]) as g:
        assert int(g.pool("segs")["name"].max()) == ps.U64_MAX


@pytest.mark.parametrize("make", [ps.digit_names, lambda: ps.alternating(40), lambda: ps.long_overlaps(50),
                                  lambda: ps.long_cigar(30, 10), lambda: ps.path_name(65)],
                         ids=["digit names", "alternating", "long overlaps", "long cigar", "path name"])
def test_builders(make):
    text = make()
    with pa.parse_bytes(text) as g:
        assert pm.gfa(pm.pools_of(g)) == g.gfa_text()
        assert len(g.gfa_text()) == len(text)


def test_pools_no_text_gives(tmp_path):
    text = ps.alternating(12)
    for p in (ps.short_line_order(text, 7), ps.normalized(text), ps.shared_steps(text), ps.normalized(ps.HANDMADE["P before S"]),
              ps.wide_ops(ps.long_cigar(30, 10)), ps.wide_ops(ps.HANDMADE["path overlaps"])):
        with load(p, tmp_path) as g:
            assert pm.gfa(p) == g.gfa_text()
    with load(ps.short_line_order(text, 7), tmp_path) as g:
        assert g.gfa_text() == b"".join(text.splitlines(True)[:7])


ERRORS = {
    "print: empty header": lambda: ps.with_pools(ps.fo.parse_gfa(ps.HANDMADE["plain"]), header=ps.np.zeros(0, ps.np.uint8)),
    "print: too few segments": lambda: ps.order_of(ps.HANDMADE["plain"], [0, 1, 1, 1, 2, 1, 3]),
    "print: too few paths": lambda: ps.order_of(ps.HANDMADE["plain"], [1, 2, 3, 2]),
    "print: too few links": lambda: ps.order_of(ps.HANDMADE["plain"], [3, 3, 3]),
    "print: bad line kind": lambda: ps.order_of(ps.HANDMADE["plain"], [1, 4]),
    "print: path with no steps": lambda: ps.path_without_steps(ps.HANDMADE["path overlaps"], 1),
}


@pytest.mark.parametrize("message", list(ERRORS))
def test_errors(message, tmp_path):
    p = ERRORS[message]()
    with pytest.raises(pm.PrintError, match=message):
        pm.gfa(p)
    with load(p, tmp_path) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            g.gfa_text()
        assert e.value.code == -2 and pa._lib.last_error() == message


# ---- the seam shapes of tests/test_gpu_print_seams.py: each is on its seam, and the model and the host printer agree on it ----

def printed(x, tmp_path) -> bytes:
    """The host printer's text of a text or of pools, which the model gives too."""
    if isinstance(x, bytes):
        with pa.parse_bytes(x) as g:
            want = g.gfa_text()
            assert want == x and pm.gfa(pm.pools_of(g)) == want
    else:
        with load(x, tmp_path) as g:
            want = g.gfa_text()
            assert pm.gfa(x) == want
    return want


@pytest.mark.parametrize("size", ps.TEXT_ENDS)
def test_text_ends(size, tmp_path):
    text = printed(ps.exact_text(size, ps.width_for(size)), tmp_path)
    assert len(text) == size and text.endswith(ps.TAIL)
    sizes = ps.item_sizes(text)
    want = {ps.PIECE: [ps.PIECE], ps.PIECE + 1: [ps.PIECE, 1], 2 * ps.PIECE: [ps.PIECE, ps.PIECE]}.get(size, [size])
    assert ps.pieces(sizes) == want and len(sizes) == text.count(b"\n") + 2  # (the tail's path has three steps)


@pytest.mark.parametrize("size", ps.CHUNK_ENDS)
def test_chunk_ends(size, tmp_path):
    made, chunk = ps.chunk_then_more(size, ps.width_for(size))
    text = printed(made, tmp_path)
    per_chunk = ps.chunk_bytes(ps.item_sizes(text), chunk)
    assert per_chunk[0] == size and len(per_chunk) > 1 and sum(per_chunk) == len(text) > size
    want = {ps.PIECE: [ps.PIECE], ps.PIECE + 1: [ps.PIECE, 1], 2 * ps.PIECE: [ps.PIECE, ps.PIECE]}.get(size, [size])
    assert ps.pieces(ps.item_sizes(text), chunk)[:len(want)] == want


def test_scan_chunk_graphs_have_more_items_than_a_chunk():
    with pa.synth(11, 2000, 4, 2000, with_seq=True) as g:
        assert len(ps.item_sizes(g.gfa_text())) == 2000 + 4 * 2000 > 2 * max(ps.SCAN_CHUNKS)
    text = ps.alternating(1500)
    assert len(ps.item_sizes(text)) == 2 + 4 * 1500 > max(ps.SCAN_CHUNKS)
    with pa.parse_bytes(text) as g:
        assert len(g.pool("line_order")) and g.gfa_text() == text


def test_item_sizes_are_the_items_of_the_design():
    """One item a line, one a step; the first and the last item of a P line carry its ends."""
    text = ps.HANDMADE["path overlaps"]  # P q 1+,2-,3+ 2M,10M3D | P r 3-,2+ 4M | P s 1+ *
    assert ps.item_sizes(text) == [9, 9, 9, 4 + 3, 3, 3 + 9, 4 + 3, 3 + 3, 4 + 3 + 2]
    assert ps.line_items(text) == [(0, 1), (1, 1), (2, 1), (3, 3), (6, 2), (8, 1)]
    assert ps.pieces([3, ps.PIECE, 1, 2 * ps.PIECE - 1, 5], 2) == [ps.PIECE, 3, ps.PIECE, ps.PIECE, 5]


@pytest.mark.parametrize("case", list(ps.cut_cases()))
def test_cut_cases(case, tmp_path):
    text = printed(ps.CUT_TEXT, tmp_path)
    chunk, items = ps.cut_cases()[case]
    sizes, lines = ps.item_sizes(text), ps.line_items(text)
    assert chunk >= 1 and set(items) <= ps.cuts(sizes, chunk)
    # the items are what the case says: the last, the second, or the only item of a P line with several alignments
    name, what = case.split(": ")
    (k,) = [k for k, ln in enumerate(text[:-1].split(b"\n")) if ln.startswith(b"P\t" + name.encode() + b"\t")]
    (first, n), ovl = lines[k], text[:-1].split(b"\n")[k].split(b"\t")[3]
    assert ovl.count(b",") >= 1 and any(len(re.findall(rb"[MNDI]", a)) > 1 for a in ovl.split(b","))
    want = {"before its last item": [first + n - 1], "behind its first item": [first + 1], "before its one item": [first],
            "behind its one item": [first + 1], "alone in a chunk": [first, first + 1]}[what]
    assert items == want and (n == 1) == ("one" in what or "alone" in what) and 0 < items[0] < len(sizes)


def test_cut_cases_cover_every_path():
    names = {c.split(":")[0] for c in ps.cut_cases()}
    assert names == {"q", "one", "r", "last"} and len(ps.cut_cases()) == 3 * 2 + 3


@pytest.mark.parametrize("case", list(ps.clipped_cases()))
def test_clipped_cases(case, tmp_path):
    make, kind, tile, want = ps.clipped_cases()[case]
    text = printed(make(), tmp_path)
    span = ps.crossing(text, kind)
    assert ps.clipped(span, tile) == want and span[2] - span[1] > 64
    if want in ps.RESTS:  # the copy is a lane's up to 64 bytes, the workgroup's above
        assert (ps.clipped(span, tile) > 64) == (want >= 65) and ps.clipped(span, 1 - tile) > 64


@pytest.mark.parametrize("case", list(ps.header_first_cases()))
def test_header_first(case, tmp_path):
    p = ps.header_first_cases()[case]()
    text = printed(p, tmp_path)
    assert len(p.line_order) == 0 and text.startswith(b"H\t" + p.header.tobytes() + b"\n") and len(p.header) > 64
    assert (len(p.header) > ps.TILE) == ("tile" in case)


@pytest.mark.parametrize("optional", [False, True])
def test_many_long_copies(optional, tmp_path):
    text = printed(ps.many_long(1000, optional), tmp_path)
    assert len(text) == 1000 * (136 if optional else 70) > 4 * ps.TILE
    full = range(1, len(text) // ps.TILE)  # tiles with text on both sides
    assert len(full) >= 3
    for tile in full:
        assert (238 if optional else 230) <= ps.long_copies(text, tile) <= ps.LONG_CAP - 2


def test_long_copy_capacity():
    """Copies of more than 64 bytes are disjoint in a tile's 16384 bytes: never more than 252 of them, under kLongCap."""
    assert ps.TILE // 65 == 252 and ps.LONG_CAP == 254


def test_aliased_segments(tmp_path):
    """The closed form of the text of aliased segments is the host printer's, at a size it can print; at 65 segments over 2^26
    bases the text passes 2^32 bytes inside the last segment but one, and the path and the link lie just behind."""
    small = ps.aliased_segments(5, 1000)
    text = printed(small, tmp_path)
    assert sum(n for n, *_ in ps.aliased_lines(small)) == len(text)
    for lo, hi in ((0, len(text)), (0, 3), (2, 1003), (1004, 1006), (1005, 2011), (4000, 4100), (len(text) - 900, len(text))):
        assert ps.aliased_window(small, lo, hi) == text[lo:hi]
    big = ps.aliased_segments(65, 1 << 26)
    lengths = [n for n, *_ in ps.aliased_lines(big)]
    assert sum(lengths) == 65 * (1 << 26) + 9 * 5 + 56 * 6 + len(b"P\tp\t1+,2-\t*\nL\t1\t+\t2\t-\t0M\n") > (1 << 32)
    assert sum(lengths[:63]) < (1 << 32) - 4096 and (1 << 32) < sum(lengths[:64]) < (1 << 32) + 4096 - 40
    window = ps.aliased_window(big, (1 << 32) - 4096, (1 << 32) + 4096)
    assert len(window) == 8192 and b"\nP\tp\t1+,2-\t*\nL\t1\t+\t2\t-\t0M\nS\t65\t" in window


@pytest.mark.parametrize("case", list(ps.degenerate_cases()))
def test_degenerate(case, tmp_path):
    x = ps.degenerate_cases()[case]()
    text = printed(x, tmp_path)
    kinds = {ln[:1] for ln in text[:-1].split(b"\n")}
    if "only S" in case:
        assert kinds == {b"S"}
    if "only L" in case:
        assert kinds == {b"L"} and text.count(b"\n") == 3 and len(x.segs) == 3
    if "6 bytes" in case:
        assert len(text) == 6 < 16
    if "empty sequence" in case:
        assert b"S\t2\t\n" in text
    if "empty path name" in case:
        assert b"P\t\t3-,2+\t4M\n" in text
    if "one-step" in case:
        assert b"P\t\t1+\t*\n" in text
