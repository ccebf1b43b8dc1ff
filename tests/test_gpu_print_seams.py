"""The device GFA printer (print_device.hip, text_tiles.hpp) at the seams its first tests leave at no pinned size: where a
text, a chunk or a piece ends (A), the chunk scan at more than one scan tile (B), chunk cuts at chosen items of a P line (C),
copies from a pool that are 63..66 bytes once clipped to a tile, the header among them (D), tiles that are nearly all long
copies (E), a text of more than 2^32 bytes (F) and degenerate graphs (G).  Every shape is built in tests/print_shapes.py,
pinned to its seam on the host by tests/test_print_model.py, and compared here with the host printer byte for byte through
the buffer call, the stream and gfa_bytes (check, from test_gpu_print_geometry.py); where the cuts matter, the piece lengths
the sink sees are compared with the ones the item sizes give.  Run with -m gpu.

Not reached, by construction: the lane's own copy behind `e < kLongCap` in put_bytes.  Copies of more than 64 clipped bytes
are disjoint stretches of a tile's 16384 bytes, so a tile has at most 16384 / 65 = 252 of them and kLongCap is 254; group E
comes as near as lines allow (234 and 241 a tile).

Group F prints 65 segments over one pool of 2^26 bases, 4 362 076 566 bytes of text from a container of 64 MiB: the size
the full size, not a halved one.  Measured on an MI355X: 0.37 s of wall time for the test, of which gfa_bytes 0.01 s and
the streamed text 0.22 s (about 20 GB/s into the sink); the rest makes the pool.  Every other test takes well under a
second (the first one carries the process's device start-up, 1.6 s).
"""
import os
import time

import pytest

import pollen_amd as pa
import print_shapes as ps
from test_gpu_print_geometry import check
from test_print_model import load

pytestmark = pytest.mark.gpu
TILE, PIECE = ps.TILE, ps.PIECE
HOOK = "FLATGFA_PRINT_CHUNK_ITEMS"


def seen(g) -> list:
    """The piece lengths a sink sees."""
    n = []
    g.gfa_stream(lambda b: n.append(len(b)))
    return n


def opened(x, tmp_path):
    return pa.parse_bytes(x) if isinstance(x, bytes) else load(x, tmp_path)


def check_cuts(g, chunk, monkeypatch):
    """With chunks of `chunk` items: the bytes are the host printer's on every route, and the sink sees the pieces that the
    items' sizes give -- so the cuts are where the test means them to be."""
    monkeypatch.setenv(HOOK, str(chunk))
    want = check(g)
    sizes = ps.item_sizes(want)
    got = seen(g)
    assert got == ps.pieces(sizes, chunk) and all(got) and len(got) >= -(-len(sizes) // chunk)
    return want, sizes


# ---- A: where the text, a chunk or a piece ends ----

@pytest.mark.parametrize("size", ps.TEXT_ENDS)
def test_text_ends(size):
    assert HOOK not in os.environ
    with pa.parse_bytes(ps.exact_text(size, ps.width_for(size))) as g:
        want = check(g)
        assert len(want) == size
        got = seen(g)
        assert got == {PIECE: [PIECE], PIECE + 1: [PIECE, 1], 2 * PIECE: [PIECE, PIECE]}.get(size, [size]) and all(got)


@pytest.mark.parametrize("size", ps.CHUNK_ENDS)
def test_chunk_ends(size, monkeypatch):
    text, chunk = ps.chunk_then_more(size, ps.width_for(size))
    with pa.parse_bytes(text) as g:
        want, sizes = check_cuts(g, chunk, monkeypatch)
        assert want == text and ps.chunk_bytes(sizes, chunk)[0] == size
        head = {PIECE: [PIECE], PIECE + 1: [PIECE, 1], 2 * PIECE: [PIECE, PIECE]}.get(size, [size])
        assert seen(g)[:len(head) + 1] == head + [len(text) - size]  # the chunk's pieces, then the rest of the text


# ---- B: the chunk scan at one, two and four scan tiles ----

@pytest.mark.parametrize("chunk", ps.SCAN_CHUNKS)
def test_scan_chunks(chunk, monkeypatch):
    with pa.synth(11, 2000, 4, 2000, with_seq=True) as g:
        _, sizes = check_cuts(g, chunk, monkeypatch)
        assert len(sizes) == 10_000
    with pa.parse_bytes(ps.alternating(1500)) as g:
        _, sizes = check_cuts(g, chunk, monkeypatch)
        assert len(sizes) == 6002 and len(g.pool("line_order"))


# ---- C: a chunk cut at a chosen item of a P line ----

@pytest.mark.parametrize("case", list(ps.cut_cases()))
def test_cuts_in_a_p_line(case, monkeypatch):
    chunk, items = ps.cut_cases()[case]
    with pa.parse_bytes(ps.CUT_TEXT) as g:
        want, sizes = check_cuts(g, chunk, monkeypatch)
        assert want == ps.CUT_TEXT and set(items) <= ps.cuts(sizes, chunk)


# ---- D: long copies at the threshold after clipping; the header as a long copy ----

@pytest.mark.parametrize("case", list(ps.clipped_cases()))
def test_clipped_long_copies(case):
    make, kind, tile, n = ps.clipped_cases()[case]
    text = make()
    with pa.parse_bytes(text) as g:
        assert check(g) == text
    assert ps.clipped(ps.crossing(text, kind), tile) == n


@pytest.mark.parametrize("case", list(ps.header_first_cases()))
def test_header_first(case, tmp_path):
    p = ps.header_first_cases()[case]()
    with load(p, tmp_path) as g:
        assert check(g).startswith(b"H\t" + p.header.tobytes() + b"\n")


# ---- E: tiles of long copies ----

@pytest.mark.parametrize("optional", [False, True])
def test_many_long_copies(optional, tmp_path):
    with load(ps.many_long(1000, optional), tmp_path) as g:
        want = check(g)
    counts = [ps.long_copies(want, t) for t in range(1, len(want) // TILE)]
    assert len(counts) >= 3 and min(counts) >= (238 if optional else 230)


# ---- F: more than 2^32 bytes of text ----

def test_past_4_gib(tmp_path):
    p = ps.aliased_segments(65, 1 << 26)
    total = sum(n for n, *_ in ps.aliased_lines(p))
    assert total == 4_362_076_566 > 1 << 32
    windows = [(0, TILE), ((1 << 32) - 4096, (1 << 32) + 4096), (total - total % TILE, total)]
    with load(p, tmp_path) as g:
        t0 = time.perf_counter()
        assert g.gfa_bytes() == total
        t1 = time.perf_counter()
        state = {"at": 0, "calls": 0}
        kept = [[] for _ in windows]

        def sink(b):
            at = state["at"]
            for (lo, hi), keep in zip(windows, kept):
                if at < hi and at + len(b) > lo:
                    keep.append(b[max(lo - at, 0):hi - at])
            state["at"], state["calls"] = at + len(b), state["calls"] + 1
        g.gfa_stream(sink)
        print("past 4 GiB: gfa_bytes %.2f s, gfa_stream %.2f s" % (t1 - t0, time.perf_counter() - t1))
    assert state["at"] == total and state["calls"] == -(-total // PIECE)  # one chunk: pieces of 4 MiB and a rest
    for (lo, hi), keep in zip(windows, kept):
        got = b"".join(keep)
        assert len(got) == hi - lo and got == ps.aliased_window(p, lo, hi), (lo, hi)
    assert b"\nP\tp\t1+,2-\t*\nL\t1\t+\t2\t-\t0M\nS\t65\t" in b"".join(kept[1])  # the short lines lie past 2^32


# ---- G: degenerate graphs ----

@pytest.mark.parametrize("case", list(ps.degenerate_cases()))
def test_degenerate(case, tmp_path):
    x = ps.degenerate_cases()[case]()
    with opened(x, tmp_path) as g:
        want = check(g)
        assert seen(g) == [len(want)]
    if isinstance(x, bytes):
        assert want == x
