"""slow_odgi/slow_odgi/crush.py on oracle.flatgfa_oracle.Pools, for the tests only, in two forms:

  crush        a loop per segment that reads like crush.py:5-17 (crush_seg), Python bytes
  crush_fast   the keep-flag rule over the bases of the segments laid end to end, in numpy: byte k of a segment is dropped
               iff it is N, k > 0 and byte k - 1 of the same segment is N

Both give the pools `fgfa crush` writes: seq_data is the crushed segments one behind another in segment order, whatever the
input's spans were; a segment keeps its name, loses its optional fields and gets the span of its bytes in the new pool (an
empty one: the empty span at the place where the next segment begins); paths keep name and steps and lose their overlaps
(crush.py:27, drop_all_overlaps); header, links, alignment, steps and name_data are the input's; overlaps, optional_data and
line_order are empty, so the text comes out in normalized order.  Only the byte 0x4E is N: the reference's parser admits only
ATGCN, and for any other byte -- n and * included -- this model decides: it is an ordinary byte.

Also here: the device code's geometry (crush_device.hpp), held against the source text by tests/test_crush_model.py.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List

import numpy as np

from oracle import flatgfa_oracle as fo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pollen_amd", "csrc")
N = 0x4E
TILE, THREADS, GRID, SCAN_PER = 16384, 256, 2048, 4
SCAN_TILE = THREADS * SCAN_PER


def source_constants() -> Dict[str, int]:
    with open(os.path.join(CSRC, "crush_device.hpp")) as f:
        s = f.read()

    def one(pat):
        m = re.search(pat, s)
        assert m, pat
        return int(m.group(1))

    return {"TILE": one(r"constexpr uint32_t kCrushTile = (\d+);"), "THREADS": one(r"constexpr int kCrushThreads = (\d+);"),
            "GRID": one(r"constexpr uint32_t kCrushGrid = (\d+);"), "SCAN_PER": one(r"constexpr uint32_t kCrushScanPer = (\d+);")}


def crush_seq(seq: bytes) -> bytes:
    """crush.py:5-17."""
    new, in_n = bytearray(), False
    for ch in seq:
        if ch == N:
            if in_n:
                continue
            in_n = True
        else:
            in_n = False
        new.append(ch)
    return bytes(new)


def _store(p: fo.Pools, seqs_len: np.ndarray, seq_data: np.ndarray) -> fo.Pools:
    end = np.cumsum(seqs_len.astype(np.int64))
    segs = np.zeros(len(p.segs), fo.SEG_DT)
    segs["name"] = p.segs["name"]
    segs["seq_start"], segs["seq_end"] = end - seqs_len, end
    paths = np.zeros(len(p.paths), fo.PATH_DT)
    for f in ("name_start", "name_end", "steps_start", "steps_end"):
        paths[f] = p.paths[f]
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=p.header, segs=segs, paths=paths, links=p.links, steps=p.steps, seq_data=seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=p.alignment, name_data=p.name_data, optional_data=z, line_order=z)


def check_spans(p: fo.Pools) -> None:
    a, b = p.segs["seq_start"].astype(np.int64), p.segs["seq_end"].astype(np.int64)
    if len(a) and ((a > b).any() or (b > len(p.seq_data)).any()):
        raise IndexError("a segment's span leaves seq_data")


def crush(p: fo.Pools) -> fo.Pools:
    """Segment by segment, as crush.py:20-22."""
    check_spans(p)
    pool = p.seq_data.tobytes()
    new: List[bytes] = [crush_seq(pool[int(s["seq_start"]):int(s["seq_end"])]) for s in p.segs]
    return _store(p, np.array([len(x) for x in new], np.int64), np.frombuffer(b"".join(new), np.uint8).copy())


def laid_out(p: fo.Pools):
    """The bases of the segments laid end to end, and for each whether it is its segment's first."""
    check_spans(p)
    start = p.segs["seq_start"].astype(np.int64)
    lens = p.segs["seq_end"].astype(np.int64) - start
    legend = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(legend[-1])
    seg = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(total, dtype=np.int64) - legend[seg]
    return p.seq_data[start[seg] + within], within == 0, seg, lens


def crush_fast(p: fo.Pools) -> fo.Pools:
    """The keep flags over the laid-out bases."""
    b, first, seg, lens = laid_out(p)
    is_n = b == N
    prev_n = np.concatenate([[False], is_n[:-1]])
    keep = ~(is_n & ~first & prev_n)
    dropped = np.bincount(seg[~keep], minlength=len(lens)).astype(np.int64)
    return _store(p, lens - dropped, b[keep].copy())


def dropped(p: fo.Pools) -> int:
    """How many bytes a crush of p drops."""
    lens = p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"].astype(np.int64)
    return int(lens.sum()) - len(crush_fast(p).seq_data)


def seg_seq(p: fo.Pools) -> np.ndarray:
    """u32[2 * S]: start and length per segment, as the device-level entry takes them."""
    out = np.zeros(2 * len(p.segs), np.uint32)
    out[0::2] = p.segs["seq_start"]
    out[1::2] = p.segs["seq_end"] - p.segs["seq_start"]
    return out


def pools_of(g) -> fo.Pools:
    """The pools of a pollen_amd FlatGFA."""
    return fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})


def assert_same_pools(got: fo.Pools, want: fo.Pools, what="") -> None:
    for n in fo.POOL_ORDER:
        assert getattr(got, n).tobytes() == getattr(want, n).tobytes(), (n, what)


def text(p: fo.Pools) -> bytes:
    """The GFA text the project's printer makes of these pools (through a .flatgfa file and flatgfa_load)."""
    import chop_model
    return chop_model.text(p)


# ---- the reference's text against this project's ----
def _flip(h: bytes) -> bytes:
    return b"-" if h == b"+" else b"+"


def norm_link(line: bytes) -> bytes:
    """An L line as the smaller of itself and its reverse (flip(to), flip(from)): the reference prints links normalised."""
    f = line.split(b"\t")
    a = (f[1], f[2], f[3], f[4])
    b = (f[3], _flip(f[4]), f[1], _flip(f[2]))
    return b"\t".join((b"L",) + min(a, b) + tuple(f[5:]))


_SWAP = bytes.maketrans(b"DI", b"ID")


def text_views(t: bytes, ours: bool = False):
    """(sorted S lines, sorted P lines, sorted normalised L lines, H lines) of a GFA text.  ours: the text is this project's
    printer's, which -- as the reference's print.rs:14-23 -- writes an insertion as D and a deletion as I in a link's
    alignment, where slow_odgi writes the letters it read; they are swapped back before the comparison."""
    lines = t.splitlines()
    if ours:
        lines = [b"\t".join(ln.split(b"\t")[:5] + [ln.split(b"\t")[5].translate(_SWAP)]) if ln[:1] == b"L" else ln for ln in lines]
    pick = lambda c: sorted(ln for ln in lines if ln[:1] == c)  # noqa: E731
    return pick(b"S"), pick(b"P"), sorted(norm_link(ln) for ln in lines if ln[:1] == b"L"), pick(b"H")
