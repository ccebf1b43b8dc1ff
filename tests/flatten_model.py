"""slow_odgi/slow_odgi/flatten.py rule by rule on oracle.flatgfa_oracle.Pools, in Python ints: the legend, the FASTA record and
the BED table that `slow_odgi flatten` prints, for the tests only.

  legend   flatten.py:13-19   ptr walks the segments in pool order; legend[s] = (ptr, ptr + len)
  FASTA    flatten.py:51-55   ">" name, print's newline; the bases glued together, "\\n".join of their 80-byte slices
                              (insert_newlines, :44-46), print's newline -- so no bases at all print as one empty line
  BED      flatten.py:23-41   the header line, then per path and per step of it, in order, with the step's index

The reference keys segments and paths by name, so it cannot say what a graph with two paths of one name flattens to; here,
as in the product, a line belongs to (path, rank) and every path is emitted.  Also here: the constants of the device code
(source_constants) as the source text has them, for the shapes that sit at tile, chunk and scan edges.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List

import numpy as np

from oracle import flatgfa_oracle as fo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pollen_amd", "csrc")
WRAP = 80
BED_HEADER = b"#name\tstart\tend\tpath.name\tstrand\tstep.rank\n"
# the device code's geometry (flatten_device.hpp); test_flatten_model.py holds them against the source text
TILE, PIECE, THREADS, SCAN_PER, CHUNK_LINES, LONG_NAME = 16384, 4 << 20, 256, 4, 1 << 20, 64
SCAN_TILE = THREADS * SCAN_PER


def source_constants() -> Dict[str, int]:
    """The same numbers as flatten_device.hpp has them."""
    with open(os.path.join(CSRC, "flatten_device.hpp")) as f:
        s = f.read()

    def one(pat):
        m = re.search(pat, s)
        assert m, pat
        return m

    piece = one(r"constexpr uint64_t kFlatPieceBytes = \(uint64_t\)(\d+) << (\d+);")
    return {
        "TILE": int(one(r"constexpr uint32_t kFlatTile = (\d+);").group(1)),
        "PIECE": int(piece.group(1)) << int(piece.group(2)),
        "THREADS": int(one(r"constexpr int kFlatThreads = (\d+);").group(1)),
        "SCAN_PER": int(one(r"constexpr uint32_t kFlatScanPer = (\d+);").group(1)),
        "CHUNK_LINES": 1 << int(one(r"constexpr uint64_t kFlatChunkLines = \(uint64_t\)1 << (\d+);").group(1)),
        "LONG_NAME": int(one(r"constexpr uint32_t kFlatLongName = (\d+);").group(1)),
        "WRAP": int(one(r"constexpr uint32_t kFlatWrap = (\d+);").group(1)),
    }


def legend(p: fo.Pools) -> List[int]:
    """flatten.py:13-19: S + 1 offsets."""
    out, ptr = [0], 0
    for sg in p.segs:
        ptr += int(sg["seq_end"]) - int(sg["seq_start"])
        out.append(ptr)
    return out


def bases(p: fo.Pools) -> bytes:
    """flatten.py:15-16: every segment's seq in pool order (the spans say where each lies; nothing else does)."""
    data = p.seq_data.tobytes()
    return b"".join(data[int(sg["seq_start"]):int(sg["seq_end"])] for sg in p.segs)


def insert_newlines(s: bytes, every: int = WRAP) -> bytes:
    """flatten.py:44-46"""
    return b"\n".join(s[i:i + every] for i in range(0, len(s), every))


def fasta(p: fo.Pools, name: bytes) -> bytes:
    """flatten.py:51-55"""
    return b">" + name + b"\n" + insert_newlines(bases(p)) + b"\n"


def bed(p: fo.Pools, name: bytes) -> bytes:
    """flatten.py:23-41"""
    leg = legend(p)
    steps = p.steps
    out = [BED_HEADER]
    for k in range(len(p.paths)):
        pname = p.path_name(k)
        for i in range(int(p.paths[k]["steps_start"]), int(p.paths[k]["steps_end"])):
            h = int(steps[i])
            out.append(b"\t".join([name, b"%d" % leg[h >> 1], b"%d" % leg[(h >> 1) + 1], pname, b"-" if h & 1 else b"+",
                                   b"%d" % (i - int(p.paths[k]["steps_start"]))]) + b"\n")
    return b"".join(out)


def flatten(p: fo.Pools, name: bytes) -> bytes:
    """What `slow_odgi flatten` prints: flatten.py:49-57."""
    return fasta(p, name) + bed(p, name)


def fasta_body_len(total: int) -> int:
    """The record's bytes behind its header line: the bases, a newline per started line."""
    return total + -(-total // WRAP) if total else 1


def bed_fast(p: fo.Pools, name: bytes) -> bytes:
    """bed() for graphs of a few hundred thousand steps (the same rules, the numbers formatted by numpy)."""
    leg = np.array(legend(p), dtype=object)
    out = [BED_HEADER]
    for k in range(len(p.paths)):
        b, e = int(p.paths[k]["steps_start"]), int(p.paths[k]["steps_end"])
        h = p.steps[b:e].astype(np.int64)
        seg = h >> 1
        pname = p.path_name(k)
        strand = np.where(h & 1, "-", "+")
        lines = [b"%s\t%d\t%d\t%s\t%s\t%d\n" % (name, leg[s], leg[s + 1], pname, sd.encode(), i)
                 for i, (s, sd) in enumerate(zip(seg.tolist(), strand.tolist()))]
        out.append(b"".join(lines))
    return b"".join(out)
