"""GAF texts shaped around the tiles of the GPU scan (pollen_amd/csrc/gaf_device.hip), for the tests only.

Every generator takes the tile size and a seed and returns a Shape: the text, names some of its lines are built to set,
and the byte offset of the first line that names a segment the graph lacks (None when there is none).  The GPU tests
build them at GPU_TILE; tests/test_pangenotype_model.py builds them with tiny tiles, where the byte-at-a-time model is
fast enough to pin the line-at-a-time one.  Features sit at `k * tile + d` for d in EDGES: around a tile's first byte,
which is also a 4 KiB step's and a 16-byte lane's.
"""
from __future__ import annotations

from typing import FrozenSet, List, NamedTuple, Optional, Tuple

import numpy as np

# The geometry of k_gaf_tiles / k_gaf_rows: kGafTile = 256 lanes x 16 bytes x kGafSteps (8) steps of 4 KiB, and a
# lookback batch reads the summaries of 64 tiles (one per lane of wave 0).
GPU_TILE = 32 * 1024
STEPS = 8
LOOKBACK = 64
EDGES = (-17, -16, -1, 0, 1, 15, 16)

# The graph every shape is read against: a sequential run (id = name - 1) and names the NameMap keeps in `others`,
# among them names at and above 2^63 and 19- and 20-digit ones.
SEQ = 48
OTHERS = (977, 5000, 5002, 123456789, 2**63 - 1, 2**63, 2**63 + 977, 2**64 - 2, 2**64 - 1)
NAMES = list(range(1, SEQ + 1)) + list(OTHERS)
UNKNOWN = (0, SEQ + 1, 976, 978, 4999, 5001, 123456788, 2**63 - 2, 2**63 + 1, 2**64 - 3, 10**12)

LONG = (2**63 - 1, 2**63, 2**64 - 2)  # 19 and 20 digits: a token of one starting at d = -17 or -16 spans the edge
LATE = (45, 46, 2**64 - 1)  # only in the last tiles of shape A's path field
F_ZEROS, F_WRAP = 47, 2**63 + 977  # only in shape F
EARLY = tuple(n for n in NAMES if n not in LONG + LATE + (F_ZEROS, F_WRAP, SEQ))
FIRST_LINE = SEQ  # the short line some shapes start with names only this


class Shape(NamedTuple):
    text: bytes
    sets: FrozenSet[int]  # names that must come out set
    exact: bool  # the row is exactly `sets`
    bad: Optional[int]  # the first bad line's offset


def gfa(names=NAMES) -> bytes:
    """A GFA whose segments carry `names` in id order, with one path (so the graph can be made resident)."""
    segs = b"".join(b"S\t%d\tACGT\n" % n for n in names)
    return b"H\tVN:Z:1.0\n" + segs + b"P\tp\t1+,2+,3-\t*\n"


def at(tile: int, k: int, d: int = 0, step: int = 0) -> int:
    """Byte d from the start of step `step` (of STEPS) of tile k."""
    return k * tile + step * (tile // STEPS) + d


class _Text:
    """A GAF text built front to back; bulk path-field bytes are '>'/'<' tokens drawn from a set of names."""

    def __init__(self, rng, names):
        self.b = bytearray()
        self.rng = rng
        self.use(names)

    def use(self, names):
        toks = []
        for _ in range(128):
            name = names[int(self.rng.integers(len(names)))]
            pre = b"<" if self.rng.random() < 0.5 else b">"
            zeros = b"0" * int(self.rng.integers(1, 3)) if self.rng.random() < 0.2 else b""
            sep = b"x" if self.rng.random() < 0.3 else b""
            toks.append(pre + zeros + str(name).encode() + sep)
        self.toks = toks
        self.block = b"".join(toks)

    @property
    def pos(self) -> int:
        return len(self.b)

    def put(self, *parts):
        for p in parts:
            self.b += p

    def pad(self, to: int, byte: bytes = b"x"):
        assert to >= self.pos, (to, self.pos)
        self.b += byte * (to - self.pos)

    def tokens(self, to: int):
        """Whole tokens up to `to`, then 'x' (which ends a token's digits)."""
        assert to >= self.pos, (to, self.pos)
        self.b += self.block * ((to - self.pos) // len(self.block))
        for t in self.toks:
            if self.pos + len(t) > to:
                break
            self.b += t
        self.pad(to)

    def every(self, names):
        self.put(b"".join(b">%d" % n for n in names))

    def first_line(self):
        self.put(b"r0\t1\t0\t1\t+\t>%d\t1\n" % FIRST_LINE)

    def line_to(self, end: int):
        """A line whose '\\n' is at `end`: a read naming bulk tokens when there is room, else 'x'es (no tabs: skipped)."""
        head = b"rE\t1\t0\t1\t+\t"
        if end - self.pos > len(head):
            self.put(head)
            self.tokens(end)
        else:
            self.pad(end)
        self.put(b"\n")

    def text(self) -> bytes:
        return bytes(self.b)


def shape_a(tile: int, seed: int) -> Shape:
    """A path field of more than two lookback batches of tiles, full of known names; LATE names only in its last four
    tiles; 19- and 20-digit names starting at, or with their digits across, tile edges."""
    rng = np.random.default_rng(seed)
    t = _Text(rng, EARLY)
    first = seed % 2 == 0
    if not first:
        t.first_line()
    t.put(b"readA\t150\t0\t150\t+\t")
    n = 2 * LOOKBACK + 20
    ks = sorted(int(k) for k in rng.choice(np.arange(3, n - 6), size=14, replace=False))
    for i, k in enumerate(ks):
        tok = b">" + str(LONG[i % len(LONG)]).encode()
        t.tokens(at(tile, k, EDGES[i % len(EDGES)]) - (len(tok) // 2 if i % 2 else 0))
        t.put(tok)
    t.tokens(at(tile, n - 4, EDGES[seed % len(EDGES)]))
    t.use(LATE)
    t.tokens(at(tile, n, EDGES[(seed + 3) % len(EDGES)]))
    t.put(b"\t60\tcg:Z:150M\n")
    return Shape(t.text(), frozenset(LATE + LONG), False, None)


def shape_b(tile: int, seed: int, tabs: int = 5) -> Shape:
    """A line whose tabs lie in five tiles, more than a lookback batch apart in two places, then a path field of known
    names.  tabs=4: the last tab is missing, so the tokens (unknown names) are in column 5.  tabs=6: a sixth tab ends an
    empty path field and the tokens (unknown names) are in column 7.  Neither twin sets anything or errs."""
    rng = np.random.default_rng(seed)
    names = (1, 2, 3, 977, 2**63, 2**64 - 1)
    t = _Text(rng, names if tabs == 5 else UNKNOWN)
    if seed % 2:
        t.first_line()
    t.put(b"readB")
    kt = (1, 3, LOOKBACK + 6, LOOKBACK + 8, 2 * LOOKBACK + 11)
    for i, k in enumerate(kt):
        t.pad(at(tile, k, EDGES[(seed + i) % len(EDGES)]))
        t.put(b"\t" if i < 4 or tabs != 4 else b"x")
    k = kt[-1] + 1
    if tabs == 6:
        t.pad(at(tile, k, EDGES[(seed + 5) % len(EDGES)]))
        t.put(b"\t")
        k += 1
    if tabs == 5:
        t.every(names)
    t.tokens(at(tile, k + 3, EDGES[(seed + 6) % len(EDGES)]))
    t.put(b"\t60\n")
    if tabs == 5:
        return Shape(t.text(), frozenset(names), False, None)
    return Shape(t.text(), frozenset((FIRST_LINE,) if seed % 2 else ()), True, None)


def shape_c(tile: int, seed: int) -> Shape:
    """A first column of more than a lookback batch, one tab, three tiles on the other five, then more than a batch of
    tokens with unknown names in column 7: six tabs settle the state before the line's start is found."""
    rng = np.random.default_rng(seed)
    t = _Text(rng, UNKNOWN)
    if seed % 2:
        t.first_line()
    t.put(b"readC")
    k = LOOKBACK + 6
    t.pad(at(tile, k, EDGES[seed % len(EDGES)]))
    t.put(b"\t")
    t.pad(at(tile, k + 3, EDGES[(seed + 2) % len(EDGES)]))
    t.put(b"150\t0\t150\t+\t\t")
    t.tokens(at(tile, k + 4 + LOOKBACK + 8, EDGES[(seed + 4) % len(EDGES)]))
    t.put(b"\n")
    return Shape(t.text(), frozenset((FIRST_LINE,) if seed % 2 else ()), True, None)


def shape_d(tile: int, seed: int, hashed: bool, first: bool, far: bool) -> Shape:
    """A line whose five tabs lie in five tiles, two tiles (far: more than a lookback batch) after its first byte, then
    three tiles of path field.  hashed: the line starts with '#' and names unknown segments -- not an error; else it
    starts with 'r' and sets what it names."""
    rng = np.random.default_rng(seed)
    names = (4, 5, 6, 5002, 2**63 - 1)
    t = _Text(rng, UNKNOWN if hashed else names)
    if not first:
        t.first_line()
    t.put(b"#readD" if hashed else b"readD")
    k = t.pos // tile + (LOOKBACK + 4 if far else 2)
    for i in range(5):
        t.pad(at(tile, k + i, EDGES[(seed + i) % len(EDGES)]))
        t.put(b"\t")
    if not hashed:
        t.every(names)
    t.tokens(at(tile, k + 7, EDGES[(seed + 5) % len(EDGES)]))
    t.put(b"\tNM:i:0\n")
    t.first_line()
    return Shape(t.text(), frozenset((FIRST_LINE,) if hashed else names + (FIRST_LINE,)), True, None)


def shape_e(tile: int, seed: int) -> Shape:
    """Lines ending at a tile's last byte, empty lines at its first, '#' lines starting at it, a 5th (or 4th) tab as
    its last byte, a '\\n' at every EDGES offset, and runs of thousands of empty lines."""
    rng = np.random.default_rng(seed)
    known = (7, 8, 9, 10, 5000, 2**63)
    t = _Text(rng, known)
    k = 1
    for i in range(3 * len(EDGES)):
        d, step = EDGES[i % len(EDGES)], int(rng.integers(0, STEPS)) if i % 3 else 0
        kind = i % 5
        edge = at(tile, k, 0, step)
        if kind == 0:  # '\n' at the last byte before the edge and at the first after it
            t.line_to(edge - 1)
            t.put(b"\n")
        elif kind == 1:  # a '#' line from the edge on, naming unknown segments
            t.line_to(edge - 1)
            t.put(b"#E\t1\t0\t1\t+\t>%d<%d\t1\n" % (UNKNOWN[i % len(UNKNOWN)], UNKNOWN[(i + 1) % len(UNKNOWN)]))
        elif kind == 2:  # the 5th tab (odd i: the 4th) the last byte before the edge
            t.line_to(edge - 40)
            t.put(b"rE\t1\t0\t1" if i % 2 else b"rE\t1\t0\t1\t+")
            t.pad(edge - 1)
            t.put(b"\t+\t" if i % 2 else b"\t")
            t.tokens(t.pos + 20)
            t.put(b"\n")
        elif kind == 3:  # a '\n' at each offset around the edge
            t.line_to(at(tile, k, d, step))
        else:  # thousands of empty lines from the offset on, across more than one tile
            t.line_to(at(tile, k, d, step) - 1)
            t.put(b"\n" * max(3000, 2 * tile + 5))
            k = t.pos // tile + 1
        k += 2
    t.line_to(t.pos + 40)
    return Shape(t.text(), frozenset(), False, None)


def shape_f(tile: int, seed: int) -> Shape:
    """A token of 100 000 zeros and then a known name, starting at an edge; a 25-digit name that wraps mod 2^64 onto a
    known name, across a tile edge."""
    rng = np.random.default_rng(seed)
    t = _Text(rng, EARLY)
    if seed % 2:
        t.first_line()
    t.put(b"readF\t1\t0\t1\t+\t")
    t.tokens(at(tile, 2, EDGES[seed % len(EDGES)]))
    t.put(b">" + b"0" * 100_000 + str(F_ZEROS).encode())
    wrap = str(F_WRAP + int(rng.integers(54_211, 542_101)) * 2**64).encode()
    assert len(wrap) == 25
    k = t.pos // tile + 2
    t.tokens(at(tile, k, EDGES[(seed + 1) % len(EDGES)]) - 12)
    t.put(b"<" + wrap)
    t.tokens(t.pos + tile + 5)
    t.put(b"\t1\n")
    return Shape(t.text(), frozenset((F_ZEROS, F_WRAP)), False, None)


def shape_g(tile: int, seed: int, first: bool) -> Shape:
    """A line with an unknown name more than a lookback batch of tiles in, between known ones; a later short line with
    an unknown name.  The error is the long line's offset."""
    rng = np.random.default_rng(seed)
    t = _Text(rng, EARLY)
    if not first:
        while t.pos < 3 * tile:
            t.line_to(t.pos + int(rng.integers(30, 200)))
    bad = t.pos
    t.put(b"readG\t1\t0\t1\t+\t")
    t.tokens(at(tile, t.pos // tile + LOOKBACK + 8, EDGES[seed % len(EDGES)]))
    t.put(b">%d" % UNKNOWN[seed % len(UNKNOWN)])
    t.tokens(t.pos + 2 * tile)
    t.put(b"\t1\n")
    for _ in range(2):
        end = t.pos + 3 * tile
        while t.pos < end:
            t.line_to(t.pos + int(rng.integers(30, 200)))
        t.put(b"readG2\t1\t0\t1\t+\t>1>%d\n" % UNKNOWN[(seed + 1) % len(UNKNOWN)])
    return Shape(t.text(), frozenset(), False, bad)


def good_shapes(tile: int, seed: int) -> List[Tuple[str, Shape]]:
    """Every shape and twin that names no unknown segment where it is read."""
    out = [("A", shape_a(tile, seed)), ("B", shape_b(tile, seed, 5)), ("B4", shape_b(tile, seed, 4)),
           ("B6", shape_b(tile, seed, 6)), ("C", shape_c(tile, seed))]
    for hashed in (True, False):
        for first in (True, False):
            for far in (True, False):
                out.append(("D%s%s%s" % ("#" if hashed else "", "_first" if first else "", "_far" if far else ""),
                            shape_d(tile, seed, hashed, first, far)))
    out += [("E", shape_e(tile, seed)), ("F", shape_f(tile, seed))]
    return out


def bad_shapes(tile: int, seed: int) -> List[Tuple[str, Shape]]:
    return [("G", shape_g(tile, seed, False)), ("G_first", shape_g(tile, seed, True))]
