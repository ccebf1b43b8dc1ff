"""The device GFA printer at the seams of its layout -- 16 KiB tiles, 4 MiB pieces, chunks of items, the 64-byte cut between
a lane's copy and the workgroup's -- each shape (tests/print_shapes.py) against the host printer by length and sha256.  Run
with -m gpu."""
import hashlib

import pytest

import pollen_amd as pa
import print_shapes as ps
from test_print_model import load

pytestmark = pytest.mark.gpu
TILE, PIECE = ps.TILE, ps.PIECE


def same(got: bytes, want: bytes):
    assert len(got) == len(want)
    assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest()


def check(g):
    want = g.gfa_text()
    same(g.gfa_text_device(), want)
    h, n = hashlib.sha256(), []
    g.gfa_stream(lambda b: (h.update(b), n.append(len(b))) and None)
    assert sum(n) == len(want) == g.gfa_bytes() and h.digest() == hashlib.sha256(want).digest()
    return want


def check_text(text):
    with pa.parse_bytes(text) as g:
        want = check(g)
        assert len(want) == len(text)
        return want


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, TILE - 9, TILE - 8, TILE - 7, 3 * TILE + 5])
def test_long_segment(n):
    """The S line's ends on, before and behind a tile's edge (its bases begin 9 bytes into the text's first tile plus the
    line before); 3 tiles + 5 bases: one item in four tiles."""
    want = check_text(ps.one_long_segment(n))
    if n == 3 * TILE + 5:
        first, last = want.index(b"S\t2\t"), want.index(b"\nS\t3\t")
        assert last // TILE - first // TILE == 3


def test_long_optional():
    check_text(ps.long_optional(TILE + TILE // 2))


@pytest.mark.parametrize("n", [63, 64, 65, 20_000])
def test_path_name(n):
    check_text(ps.path_name(n))


def test_digit_names():
    want = check_text(ps.digit_names())
    assert str(ps.U64_MAX).encode() + b"+" in want or str(ps.U64_MAX).encode() + b"-" in want


def test_p_line_across_a_piece():
    with pa.synth(7, 20_000, 4, 700_000) as g:
        want = check(g)
        assert max(len(ln) for ln in want.split(b"\n")) > PIECE
        g.to_device(0)
        same(g.gfa_text_device(), want)


@pytest.mark.parametrize("chunk", [1, 7, 257, 1000])
def test_chunk_cuts(chunk, monkeypatch):
    """The chunk cuts move, the text does not (FLATGFA_PRINT_CHUNK_ITEMS is a test hook)."""
    with pa.synth(11, 300, 3, 700, with_seq=True) as g:
        want = g.gfa_text()
        monkeypatch.setenv("FLATGFA_PRINT_CHUNK_ITEMS", str(chunk))
        sizes = []
        g.gfa_stream(lambda b: sizes.append(len(b)))
        items = 300 + 3 * 700
        assert sum(sizes) == len(want) and len(sizes) >= items // chunk  # at least a piece per chunk
        same(g.gfa_text_device(), want)
    with pa.parse_bytes(ps.alternating(60)) as g:
        same(g.gfa_text_device(), g.gfa_text())


def test_long_overlaps():
    want = check_text(ps.long_overlaps(4000))
    assert len(want.split(b"\n")[3].split(b"\t")[3]) > TILE


@pytest.mark.parametrize("lead", [TILE - 40, TILE - 300, 2 * TILE - 1000])
def test_long_cigar_across_a_tile_edge(lead):
    text = ps.long_cigar(700, lead)
    want = check_text(text)
    start = want.index(b"L\t1\t+\t2\t-\t") + 10
    end = want.index(b"\n", start)
    assert start // TILE != end // TILE


def test_wide_ops(tmp_path):
    with load(ps.wide_ops(ps.long_cigar(700, TILE - 300)), tmp_path) as g:
        check(g)
    with load(ps.wide_ops(ps.long_overlaps(4000)), tmp_path) as g:
        check(g)


def test_alternating_kinds():
    want = check_text(ps.alternating(3000))  # 9001 lines, more than one scan tile of them, and several text tiles
    assert len(want) > 4 * TILE


def test_short_line_order_and_shared_steps(tmp_path):
    text = ps.alternating(3000)
    for p in (ps.short_line_order(text, 4001), ps.shared_steps(text), ps.normalized(text)):
        with load(p, tmp_path) as g:
            check(g)
    with load(ps.short_line_order(text, 4001), tmp_path) as g:
        assert g.gfa_text_device() == b"".join(text.splitlines(True)[:4001])
