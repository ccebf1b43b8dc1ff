"""Graphs shaped around the tiles, pieces, chunks and scans of the GPU flatten (pollen_amd/csrc/flatten_device.hip), for the
tests only: the smallest at which each kernel can go wrong.

k_flat_fasta and k_flat_bed own TILE consecutive output bytes per workgroup -- of the FASTA's body (what follows ">NAME\\n") and
of a chunk's lines (what follows the header line; a chunk is CHUNK_LINES lines, or what FLATGFA_FLATTEN_CHUNK_LINES says) --
and a launch writes PIECE bytes; the legend and the line offsets are scans in tiles of SCAN_TILE elements.  Every shape
asserts its own premise on what tests/flatten_model.py says of it: that the newline really falls on the tile edge.

The numbers come from flatten_model.source_constants(), so a changed tile moves the shapes with it.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import numpy as np

import chop_shapes as cs
import flatten_model as fm
from oracle import flatgfa_oracle as fo

_C = fm.source_constants()
TILE, PIECE, SCAN_TILE, WRAP = _C["TILE"], _C["PIECE"], _C["THREADS"] * _C["SCAN_PER"], _C["WRAP"]


class Shape(NamedTuple):
    name: str
    pools: fo.Pools
    nm: bytes = b"g.og"            # NAME
    fasta: bool = True             # the FASTA is asked for too (not where the bases add up to a gigabyte)
    chunk: Optional[int] = None    # FLATGFA_FLATTEN_CHUNK_LINES
    chunks: Optional[int] = None   # ... and how many chunks that makes


def bases(rng, n):
    return np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n)]


def graph(rng, lens, steps=None, spans=None) -> fo.Pools:
    """Segments of `lens` one behind another in seq_data (random bases); by default one path over every segment, forward."""
    lens = np.asarray(lens, dtype=np.int64)
    if steps is None:
        steps = (np.arange(len(lens), dtype=np.int64) << 1)[:2000]
    if spans is None:
        spans = [(0, len(steps))]
    p = cs.make_pools(lens, steps, spans)
    p.seq_data = bases(rng, int(lens.sum())).copy()
    return p


def body_of(p: fo.Pools) -> bytes:
    """The FASTA behind its header line: what the tiles of k_flat_fasta cover."""
    return fm.fasta(p, b"")[2:]


def lines_of(p: fo.Pools, nm: bytes) -> bytes:
    """The BED behind its header line: what the tiles of k_flat_bed cover when the table is one chunk."""
    return fm.bed(p, nm)[len(fm.BED_HEADER):]


def total_for_body(body: int) -> int:
    """The number of bases whose FASTA body has `body` bytes."""
    for t in range(max(body - body // WRAP - 2, 0), body + 1):
        if fm.fasta_body_len(t) == body:
            return t
    raise AssertionError(f"no number of bases gives a body of {body} bytes")


# ---- FASTA ----
def f_total(t: int) -> Shape:
    rng = np.random.default_rng(t)
    lens = [t] if t < 2 else [t // 2, 0, t - t // 2]
    p = graph(rng, lens)
    assert len(body_of(p)) == fm.fasta_body_len(t)
    return Shape(f"F_total_{t}", p)


def f_body_end(d: int) -> Shape:
    """The body ends d bytes past the second tile edge (d = 0: exactly at it)."""
    rng = np.random.default_rng(10 + d)
    t = total_for_body(2 * TILE + d)
    lens = rng.multinomial(t, np.ones(37) / 37)
    p = graph(rng, lens)
    assert len(body_of(p)) == 2 * TILE + d
    return Shape(f"F_body_end_{d:+d}", p)


def f_wrap_on_edges() -> Shape:
    """A wrap newline as the last byte of a tile and another as the first byte of a tile: 81 and TILE are coprime, so the first
    is the byte before tile 81 and the second lies within the first 81 tiles."""
    rng = np.random.default_rng(20)
    first = next(n for n in range(1, WRAP + 2) if (n * TILE) % (WRAP + 1) == WRAP)
    t = (WRAP + 1) * TILE + 1000
    lens = rng.integers(0, 200, 2 * t // 199 + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), t))]
    p = graph(rng, lens)
    body = body_of(p)
    last = (WRAP + 1) * TILE - 1
    assert len(body) > last + 2 and body[last] == 10 and last % (WRAP + 1) == WRAP
    assert body[first * TILE] == 10 and (first * TILE) % (WRAP + 1) == WRAP
    return Shape("F_wrap_on_edges", p)


def f_long_segment() -> Shape:
    """One segment of three tiles and a byte that starts in the middle of a tile."""
    rng = np.random.default_rng(21)
    p = graph(rng, [TILE // 3, 3 * TILE + 1, 7])
    return Shape("F_long_segment", p)


def f_empty_run() -> Shape:
    """5000 segments of no bases between the base that is the last byte of tile 0 and the base that is the first of tile 1."""
    rng = np.random.default_rng(22)
    q = TILE - 1
    assert q % (WRAP + 1) != WRAP and (q + 1) % (WRAP + 1) != WRAP
    b = q - q // (WRAP + 1)
    lens = np.concatenate([[b + 1], np.zeros(5000, np.int64), [100]])
    p = graph(rng, lens)
    leg = fm.legend(p)
    assert leg[1] == b + 1 == leg[5001] and len(body_of(p)) > TILE
    return Shape("F_empty_run", p)


def f_alias_backwards() -> Shape:
    """Spans that alias one another, run backwards through seq_data and leave gaps."""
    rng = np.random.default_rng(23)
    spans = [(200, 300), (100, 250), (0, 120), (50, 50), (0, 300), (10, 20), (299, 300), (0, 1)]
    p = graph(rng, [e - b for b, e in spans])
    p.seq_data = bases(rng, 300).copy()
    p.segs["seq_start"], p.segs["seq_end"] = [b for b, _ in spans], [e for _, e in spans]
    return Shape("F_alias_backwards", p)


def f_scan(n: int) -> Shape:
    """n segments: the legend's scan at its tile."""
    rng = np.random.default_rng(24 + n)
    p = graph(rng, rng.integers(0, 6, n))
    return Shape(f"F_scan_{n}", p)


def f_pieces() -> Shape:
    """A body of more than two pieces: nine segments over one stretch of seq_data."""
    rng = np.random.default_rng(25)
    n = PIECE // 4 + 12345
    p = graph(rng, [n] * 9)
    p.seq_data = bases(rng, n + 8).copy()
    p.segs["seq_start"] = np.arange(9) % 8
    p.segs["seq_end"] = p.segs["seq_start"] + n
    assert fm.fasta_body_len(9 * n) > 2 * PIECE
    return Shape("F_pieces", p)


# ---- BED ----
def b_offsets() -> Shape:
    """start and end cross 9 -> 10, 99 -> 100 and 999 999 999 -> 1 000 000 000: a hundred segments share ten million bases."""
    rng = np.random.default_rng(30)
    big = 10_000_000
    lens = [9, 1, 89, 1] + [big] * 99 + [999_999_999 - 100 - 99 * big, 1, 5]
    segs = np.arange(len(lens))
    steps = np.concatenate([segs << 1, (segs[::-1] << 1) | 1])
    p = cs.make_pools(lens, steps, [(0, len(steps))])
    p.seq_data = np.full(big, ord("C"), np.uint8)
    p.segs["seq_start"], p.segs["seq_end"] = 0, lens
    leg = fm.legend(p)
    assert {9, 10, 99, 100, 999_999_999, 1_000_000_000} <= set(leg) and leg[-1] == 1_000_000_005
    return Shape("B_offsets", p, fasta=False)


def b_ranks() -> Shape:
    """Ranks cross 9 / 10 and 9 999 / 10 000."""
    rng = np.random.default_rng(31)
    steps = cs.handles(rng, rng.integers(0, 50, 10_003))
    return Shape("B_ranks", graph(rng, rng.integers(0, 9, 50), steps, [(0, 10_003), (3, 14)]))


def _name_length(p: fo.Pools, at: int, want: int, what: str) -> bytes:
    """The shortest NAME (of 'n's) with which byte `at` of the lines is `want`: a name one byte longer moves line i by i bytes."""
    lines = [ln + b"\n" for ln in lines_of(p, b"").split(b"\n")[:-1]]
    first = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])[:-1]])
    for n in range(0, 400):
        starts = first + np.arange(len(lines)) * n
        i = int(np.searchsorted(starts, at, side="right")) - 1
        rel = at - int(starts[i])
        if rel >= n and rel - n < len(lines[i]) and lines[i][rel - n] == want:
            return b"n" * n
    raise AssertionError(f"no NAME length puts {what}")


def b_edge(kind: str) -> Shape:
    """A line that ends on a tile's last byte (newline), a tab that is a tile's last byte (tab_last) or the next tile's first
    (tab_first): the NAME's length shifts the lines until it does."""
    rng = np.random.default_rng(32)
    steps = cs.handles(rng, rng.integers(0, 300, 3000))
    p = graph(rng, rng.integers(0, 2000, 300), steps, [(0, 1500), (1500, 3000)])
    want, at = {"newline": (10, TILE - 1), "tab_last": (9, TILE - 1), "tab_first": (9, TILE)}[kind]
    nm = _name_length(p, at, want, kind)
    t = lines_of(p, nm)
    assert len(t) > 2 * TILE and t[at] == want
    return Shape(f"B_edge_{kind}", p, nm)


def b_long(which: str) -> Shape:
    """A path name (or the NAME) of three tiles and a byte: every line is longer than a tile."""
    rng = np.random.default_rng(33)
    steps = cs.handles(rng, rng.integers(0, 20, 9))
    p = graph(rng, rng.integers(0, 9, 20), steps, [(0, 5), (5, 9)])
    long = bytes(rng.integers(ord("a"), ord("z") + 1, 3 * TILE + 1, dtype=np.uint8))
    if which == "name":
        return Shape("B_long_name", p, long)
    p.name_data = np.frombuffer(b"q" + long, np.uint8).copy()
    p.paths["name_start"], p.paths["name_end"] = [1, 0], [1 + len(long), 1]
    return Shape("B_long_path_name", p, b"x")


def b_names_mixed() -> Shape:
    """Path names of no byte, of LONG_NAME - 1, LONG_NAME, LONG_NAME + 1 bytes and of half a tile, many lines each: the lane's own
    copy, the workgroup's, and both clipped at tile edges."""
    rng = np.random.default_rng(34)
    ln = _C["LONG_NAME"]
    sizes = [0, ln - 1, ln, ln + 1, TILE // 2, 3]
    steps = cs.handles(rng, rng.integers(0, 40, 60 * len(sizes)))
    p = graph(rng, rng.integers(0, 99, 40), steps, [(60 * k, 60 * k + 60) for k in range(len(sizes))])
    p.name_data = rng.integers(ord("A"), ord("Z") + 1, sum(sizes), dtype=np.uint8)
    ends = np.cumsum(sizes)
    p.paths["name_start"], p.paths["name_end"] = ends - sizes, ends
    return Shape("B_names_mixed", p, b"y" * (ln + 5))


def b_empty_name() -> Shape:
    rng = np.random.default_rng(35)
    return Shape("B_empty_name", graph(rng, rng.integers(0, 9, 30)), b"")


def b_spans() -> Shape:
    """A path of no steps between two that have some, two paths over one span, a path inside another, a step no path walks."""
    rng = np.random.default_rng(36)
    steps = cs.handles(rng, rng.integers(0, 30, 40))
    return Shape("B_spans", graph(rng, rng.integers(0, 9, 30), steps, [(0, 10), (10, 10), (10, 25), (10, 25), (12, 14), (0, 0), (26, 40), (40, 40)]))


def b_scan(n: int) -> Shape:
    """n lines in all: the line lengths' scan at its tile."""
    rng = np.random.default_rng(37 + n)
    steps = cs.handles(rng, rng.integers(0, 30, n))
    return Shape(f"B_scan_{n}", graph(rng, rng.integers(0, 9, 30), steps, [(0, n // 3), (n // 3, n)]))


def b_seam(chunk: int) -> Shape:
    """Paths of 7 and 5 steps in chunks of `chunk` lines: 7 cuts exactly between the paths, 4 inside both, 11 leaves a last chunk of
    one line, 1 makes every line a chunk."""
    rng = np.random.default_rng(38)
    steps = cs.handles(rng, rng.integers(0, 30, 12))
    return Shape(f"B_seam_{chunk}", graph(rng, rng.integers(0, 99, 30), steps, [(0, 7), (7, 12)]), chunk=chunk, chunks=-(-12 // chunk))


def b_seam_tiles() -> Shape:
    """Chunks of a little over a tile's worth of lines, so that chunks end inside tiles and tiles inside chunks, over three paths."""
    rng = np.random.default_rng(39)
    steps = cs.handles(rng, rng.integers(0, 300, 5000))
    p = graph(rng, rng.integers(0, 5000, 300), steps, [(0, 1700), (1700, 1701), (1701, 5000)])
    chunk = 1000
    assert len(lines_of(p, b"g.og")) // 5 > TILE
    return Shape("B_seam_tiles", p, chunk=chunk, chunks=5)


CATALOG: Dict[str, Callable[[], Shape]] = {}
for _t in (0, 79, 80, 81):
    CATALOG[f"F_total_{_t}"] = lambda t=_t: f_total(t)
for _d in (-1, 0, 1):
    CATALOG[f"F_body_end_{_d:+d}"] = lambda d=_d: f_body_end(d)
CATALOG.update({"F_wrap_on_edges": f_wrap_on_edges, "F_long_segment": f_long_segment, "F_empty_run": f_empty_run,
                "F_alias_backwards": f_alias_backwards, "F_pieces": f_pieces})
for _n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
    CATALOG[f"F_scan_{_n}"] = lambda n=_n: f_scan(n)
CATALOG.update({"B_offsets": b_offsets, "B_ranks": b_ranks, "B_long_name": lambda: b_long("name"), "B_long_path_name": lambda: b_long("path"),
                "B_names_mixed": b_names_mixed, "B_empty_name": b_empty_name, "B_spans": b_spans, "B_seam_tiles": b_seam_tiles})
for _k in ("newline", "tab_last", "tab_first"):
    CATALOG[f"B_edge_{_k}"] = lambda k=_k: b_edge(k)
for _n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
    CATALOG[f"B_scan_{_n}"] = lambda n=_n: b_scan(n)
for _c in (7, 4, 11, 1):
    CATALOG[f"B_seam_{_c}"] = lambda c=_c: b_seam(c)


def bad_handle() -> fo.Pools:
    """The last step of the second path names the first segment past the end."""
    rng = np.random.default_rng(40)
    steps = cs.handles(rng, rng.integers(0, 30, 3000))
    steps[-1] = 30 << 1
    return graph(rng, rng.integers(0, 9, 30), steps, [(0, 1000), (1000, 3000)])
