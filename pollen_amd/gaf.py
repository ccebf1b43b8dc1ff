"""The reads of a GAF file looked up in a graph, mirroring the reference's Python bindings (cucapra/pollen
flatgfa-py/flatgfa.pyi:65-78, flatgfa-py/src/lib.rs:510-605): ``graph.all_reads(gaf)`` iterates over ``GAFLine``s, a line over
its ``ChunkEvent``s.  All of them are views over the arrays of ONE ``flatgfa_gaf_events`` call (the walk runs on the GPU);
names and bases are cut from the host's copies when asked for.
"""
from __future__ import annotations

import ctypes
from typing import Iterator, List, Tuple

import numpy as np

from . import _lib
from .views import Handle

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")  # flatgfa.rs:327-345
_U64 = (1 << 64) - 1
KIND_NONE, KIND_ALL, KIND_PARTIAL = 0, 1, 2


class flatgfa_gaf_events_t(ctypes.Structure):
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("line_first", ctypes.c_void_p),
                ("name_off", ctypes.c_void_p), ("name_len", ctypes.c_void_p), ("handle", ctypes.c_void_p),
                ("kind", ctypes.c_void_p), ("a", ctypes.c_void_p), ("b", ctypes.c_void_p)]


def _array(ptr, n: int, dtype) -> np.ndarray:
    if not n:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


class ChunkEvent:
    """One token of a read's path: its handle and the stretch of the segment the read covers (gaf.rs:136-148)."""

    def __init__(self, reads: "GAFReads", k: int, index: int):
        self._r, self._k, self.index = reads, int(k), int(index)

    @property
    def handle(self) -> Handle:
        return Handle(self._r._pools, int(self._r.handles[self._k]))

    @property
    def kind(self) -> int:
        return int(self._r.kinds[self._k])

    def _len(self) -> int:
        s = self._r._pools.segs[int(self._r.handles[self._k]) >> 1]
        return int(s["seq_end"]) - int(s["seq_start"])

    @property
    def range(self) -> Tuple[int, int]:
        """flatgfa-py/src/lib.rs:527-537: None is (1, 0), All is (0, len - 1), Partial(a, b) is (a, b)."""
        if self.kind == KIND_NONE:
            return (1, 0)
        if self.kind == KIND_ALL:
            return (0, (self._len() - 1) & _U64)
        return (int(self._r.a[self._k]), int(self._r.b[self._k]))

    def sequence(self) -> str:
        """gaf.rs:158-166: the bases of the range as the graph spells them, reversed and complemented for a backward handle."""
        if self.kind == KIND_NONE:
            return ""
        bits = int(self._r.handles[self._k])
        s = self._r._pools.segs[bits >> 1]
        seq = self._r._pools.seq_data[int(s["seq_start"]):int(s["seq_end"])].tobytes()
        a, b = (0, len(seq)) if self.kind == KIND_ALL else (int(self._r.a[self._k]), int(self._r.b[self._k]))
        if a > b or b > len(seq):
            raise IndexError(f"range {a}..{b} cannot be sliced from a segment of {len(seq)} bases (the reference panics)")
        if bits & 1:
            return seq[len(seq) - b:len(seq) - a].translate(_COMP)[::-1].decode("latin-1")
        return seq[a:b].decode("latin-1")

    def segment_range(self) -> str:
        """ChunkEvent::get_seg (gaf.rs:167-197)."""
        if self.kind == KIND_NONE:
            return f"{self.index}: (skipped)"
        if self.kind == KIND_ALL:
            return f"{self.index}: {self.handle}, {self._len()}bp"
        return f"{self.index}: {self.handle}, {int(self._r.a[self._k])}-{int(self._r.b[self._k])}bp"

    def __repr__(self) -> str:
        return f"ChunkEvent({self.segment_range()})"


class GAFLine:
    """One read: its name and its events (flatgfa.pyi:70-75)."""

    def __init__(self, reads: "GAFReads", line: int):
        self._r, self._l = reads, int(line)

    @property
    def name(self) -> str:
        return self._r.name_bytes(self._l).decode(errors="replace")

    def __len__(self) -> int:
        return int(self._r.line_first[self._l + 1] - self._r.line_first[self._l])

    def __iter__(self) -> Iterator[ChunkEvent]:
        first = int(self._r.line_first[self._l])
        return (ChunkEvent(self._r, first + i, i) for i in range(len(self)))

    @property
    def chunks(self) -> List[ChunkEvent]:
        return list(self)

    def sequence(self) -> str:
        return "".join(e.sequence() for e in self)

    def segment_ranges(self) -> str:  # flatgfa-py/src/lib.rs:594-601: a newline BEFORE every event
        return "".join("\n" + e.segment_range() for e in self)


class GAFReads:
    """The answer of one flatgfa_gaf_events call; iterates over its lines (the reference's GAFParser)."""

    def __init__(self, graph, pools, ev: flatgfa_gaf_events_t, text: np.ndarray):
        self._graph, self._pools = graph, pools
        L, E = int(ev.n_lines), int(ev.n_events)
        self.line_first = _array(ev.line_first, L + 1, np.uint64)
        # names: one copy of the name bytes laid end to end (the text may be a mapping that goes when the call returns); a
        # line's name is cut from it when asked for
        off, ln = _array(ev.name_off, L, np.uint64), _array(ev.name_len, L, np.uint64)
        self._name_first = np.zeros(L + 1, dtype=np.int64)
        np.cumsum(ln.astype(np.int64), out=self._name_first[1:])
        idx = np.repeat(off.astype(np.int64) - self._name_first[:-1], ln.astype(np.int64)) + np.arange(int(self._name_first[-1]), dtype=np.int64)
        self._name_bytes = text[idx].tobytes() if L else b""
        self.handles = _array(ev.handle, E, np.uint32)
        self.kinds = _array(ev.kind, E, np.uint8)
        self.a = _array(ev.a, E, np.uint64)
        self.b = _array(ev.b, E, np.uint64)

    def name_bytes(self, line: int) -> bytes:
        return self._name_bytes[int(self._name_first[line]):int(self._name_first[line + 1])]

    def __len__(self) -> int:
        return len(self._name_first) - 1

    def __getitem__(self, i: int) -> GAFLine:
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return GAFLine(self, i % len(self))

    def __iter__(self) -> Iterator[GAFLine]:
        return (GAFLine(self, i) for i in range(len(self)))


def all_reads(graph, pools, h, text: np.ndarray) -> GAFReads:
    from .flatgfa import _check
    out = ctypes.POINTER(flatgfa_gaf_events_t)()
    _check(_lib.lib().flatgfa_gaf_events(h, text.ctypes.data if text.size else None, text.size, ctypes.byref(out)), "all_reads")
    try:
        return GAFReads(graph, pools, out.contents, text)
    finally:
        _lib.lib().flatgfa_gaf_events_free(out)
