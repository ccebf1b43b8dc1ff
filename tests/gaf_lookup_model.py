"""A plain-Python restatement of the reference's GAF lookup, for the tests only.

cucapra/pollen flatgfa/src/ops/gaf.rs (GAFLineParser, PathParser, PathChunker, ChunkEvent), flatgfa/src/memfile.rs:51-63
(MemchrSplit), flatgfa/src/cli/cmds.rs:311-376 (`fgfa gaf`), flatgfa/src/flatgfa.rs:295-345 (oriented sequences) and
flatgfa-py/src/lib.rs:527-537 (ChunkEvent.range), rule by rule; the product (pollen_amd/) never imports it.  All arithmetic
is the release build's: usize = u64, wrapping.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from gaf_model import U64, lookup, name_map

TAB = 9
NONE, ALL, PARTIAL = 0, 1, 2
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")  # flatgfa.rs:327-345: every other byte maps to itself


class ParsePanic(Exception):
    """Where GAFLineParser::parse panics: an unwrap on None, the assert at gaf.rs:45, or buf[pos] one past the line."""


class LookupError_(Exception):
    """What the library reports: `code` is "parse" (FLATGFA_ERR_PARSE) or "bounds" (FLATGFA_ERR_BOUNDS), `offset` the byte
    offset of the line."""

    def __init__(self, code: str, offset: int):
        super().__init__(f"{code} at {offset}")
        self.code, self.offset = code, offset


class Graph:
    """What the lookup reads of a graph: per segment its name and its sequence, in id order."""

    def __init__(self, seg_names: Sequence[int], seqs: Sequence[bytes]):
        self.names = [int(n) for n in seg_names]
        self.seqs = list(seqs)
        self.nm = name_map(self.names)

    @classmethod
    def from_gfa(cls, text: bytes) -> "Graph":
        names, seqs = [], []
        for ln in text.split(b"\n"):
            if ln.startswith(b"S\t"):
                f = ln.split(b"\t")
                names.append(int(f[1]))
                seqs.append(f[2])
        return cls(names, seqs)


# ---- lines (memfile.rs:51-63, gaf.rs:84-91) ----

def lines(text: bytes) -> List[Tuple[int, bytes]]:
    """(offset, line) for the bytes before every '\\n'; what follows the last one is not a line; nothing is skipped."""
    out, start = [], 0
    while True:
        pos = text.find(b"\n", start)
        if pos < 0:
            return out
        out.append((start, text[start:pos]))
        start = pos + 1


# ---- fields (gaf.rs:18-71), step by step ----

class _LineParser:
    def __init__(self, buf: bytes):
        self.buf = buf

    def next_field(self) -> Optional[bytes]:  # gaf.rs:27-32
        end = self.buf.find(b"\t")
        if end < 0:
            return None
        res, self.buf = self.buf[:end], self.buf[end + 1:]
        return res

    def skip_fields(self, n: int) -> Optional[bool]:  # gaf.rs:34-40
        for _ in range(n):
            end = self.buf.find(b"\t")
            if end < 0:
                return None
            self.buf = self.buf[end + 1:]
        return True

    def int_field(self) -> Optional[int]:  # gaf.rs:42-48
        val, pos = parse_int(self.buf, 0)
        if pos >= len(self.buf):  # buf[pos] indexes one past the line
            raise ParsePanic("index past the line")
        if self.buf[pos] not in (9, 10):  # the assert at :45
            raise ParsePanic("assert")
        self.buf = self.buf[pos + 1:]
        return val


def parse_int(b: bytes, index: int) -> Tuple[Optional[int], int]:
    """gaf.rs:264-285: (the digits from `index` on as a wrapping u64, or None when there is none; the index behind them)."""
    num, first = 0, True
    while index < len(b) and 48 <= b[index] <= 57:
        num = (num * 10 + (b[index] - 48)) & U64
        index += 1
        first = False
    return (None if first else num), index


def parse_line(line: bytes) -> Tuple[bytes, int, int, bytes]:
    """GAFLineParser::parse (gaf.rs:50-70): (name, start, end, path), or ParsePanic."""
    if not line:  # :51
        raise ParsePanic("empty")
    p = _LineParser(line)
    name = p.next_field()  # :53
    if name is None:
        raise ParsePanic("unwrap")
    p.skip_fields(4)  # :54 (the result is ignored)
    path = p.next_field()  # :57
    if path is None:
        raise ParsePanic("unwrap")
    p.skip_fields(1)  # :60 (ignored too)
    start = p.int_field()  # :61
    if start is None:
        raise ParsePanic("unwrap")
    end = p.int_field()  # :62
    if end is None:
        raise ParsePanic("unwrap")
    return name, start, end, path


def accepts(line: bytes) -> bool:
    """The closed rule: at least 9 tabs, and fields 7 and 8 are each one or more ASCII digits (a tab follows each)."""
    f = line.split(b"\t")
    return len(f) >= 10 and all(len(x) > 0 and all(48 <= c <= 57 for c in x) for x in (f[7], f[8]))


# ---- path tokens (gaf.rs:287-308) ----

def tokens(path: bytes) -> List[Tuple[int, bool]]:
    """(name, forward) per token; the walk stops, without an error, at the first byte that continues none."""
    out, i = [], 0
    while i < len(path):  # :291
        b = path[i]
        i += 1
        if b == 62:
            fwd = True
        elif b == 60:
            fwd = False
        else:
            return out  # :301
        num, i = parse_int(path, i)
        if num is None:
            return out  # :305 (`?`)
        out.append((num, fwd))
    return out


# ---- chunk events (gaf.rs:200-243) ----

def events(g: Graph, start: int, end: int, toks: Sequence[Tuple[int, bool]]):
    """[(handle, kind, a, b)] for a read, or None where the lookup panics (namemap.rs:27-33, the index into segs)."""
    out, pos, started, ended = [], 0, False, False
    for name, fwd in toks:
        sid = lookup(g.nm, name)
        if sid is None or sid >= len(g.names):
            return None
        ln = len(g.seqs[sid])
        nxt = (pos + ln) & U64
        if not started and start < nxt:
            started = True
            if end < nxt:
                ended = True
                rng = (PARTIAL, (start - pos) & U64, (end - pos) & U64)
            else:
                rng = (PARTIAL, (start - pos) & U64, ln)
        elif started and not ended and end < nxt:
            ended = True
            rng = (PARTIAL, 0, (end - pos) & U64)
        elif started and not ended:
            rng = (ALL, 0, ln)
        else:
            rng = (NONE, 0, 0)
        pos = nxt
        out.append(((sid << 1) | (0 if fwd else 1),) + rng)
    return out


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def event_bases(g: Graph, ev) -> Optional[bytes]:
    """ChunkEvent::get_seq_string (gaf.rs:158-166); None where the slice panics."""
    handle, kind, a, b = ev
    seq = g.seqs[handle >> 1]
    if kind == NONE:
        return b""
    if kind == ALL:
        a, b = 0, len(seq)
    elif a > b or b > len(seq):
        return None
    if handle & 1:  # flatgfa.rs:295-345: seq[len - b .. len - a], reversed and complemented
        return revcomp(seq[len(seq) - b:len(seq) - a])
    return seq[a:b]


def py_range(g: Graph, ev) -> Tuple[int, int]:
    """ChunkEvent.range in Python (flatgfa-py/src/lib.rs:527-537)."""
    handle, kind, a, b = ev
    if kind == NONE:
        return (1, 0)
    if kind == ALL:
        return (0, (len(g.seqs[handle >> 1]) - 1) & U64)  # (sic)
    return (a, b)


def event_text(g: Graph, index: int, ev) -> bytes:
    """ChunkEvent::get_seg (gaf.rs:167-197); the orientation prints as + or - (print.rs:4-11)."""
    handle, kind, a, b = ev
    if kind == NONE:
        return b"%d: (skipped)" % index
    head = b"%d: %d%s, " % (index, g.names[handle >> 1], b"-" if handle & 1 else b"+")
    if kind == ALL:
        return head + b"%dbp" % len(g.seqs[handle >> 1])
    return head + b"%d-%dbp" % (a, b)


# ---- the whole lookup, with the library's error rule ----

def reads(g: Graph, text: bytes, want_bases: bool = False):
    """[(name, events)] per line.  The first bad line (a parse panic; an unknown name; with want_bases, a range that cannot be
    sliced) raises LookupError_ with its offset: lines are walked in order, so it is the one at the lowest offset."""
    out = []
    for off, line in lines(text):
        try:
            name, start, end, path = parse_line(line)
        except ParsePanic:
            raise LookupError_("parse", off) from None
        evs = events(g, start, end, tokens(path))
        if evs is None:
            raise LookupError_("bounds", off)
        if want_bases and any(event_bases(g, e) is None for e in evs):
            raise LookupError_("bounds", off)
        out.append((name, evs))
    return out


def seqs_text(g: Graph, text: bytes) -> bytes:
    """`fgfa gaf -s` (cmds.rs:349-357)."""
    return b"".join(name + b"\t" + b"".join(event_bases(g, e) for e in evs) + b"\n" for name, evs in reads(g, text, True))


def table_text(g: Graph, text: bytes) -> bytes:
    """`fgfa gaf` (cmds.rs:367-374): print!, not println! -- events run together and the next name follows them directly."""
    return b"".join(name + b"\n" + b"".join(event_text(g, i, e) for i, e in enumerate(evs)) for name, evs in reads(g, text))


def count(g: Graph, text: bytes) -> Tuple[int, int]:
    """`fgfa gaf -b`: (events, lines)."""
    r = reads(g, text)
    return sum(len(evs) for _, evs in r), len(r)
