"""slow_odgi/slow_odgi/flip.py on oracle.flatgfa_oracle.Pools, for the tests only: one function per rule of the contract
(include/flatgfa.h, flatgfa_flip), then `flip`, which puts them together into the pools `fgfa flip` writes.

  weigh / turned      rule 1: a path turns iff its backward steps cover strictly more bases than its forward ones (flip.py:6-16)
  new_steps           rule 2: a turned path's steps reversed, every orientation toggled (flip.py:24-26); the pool is the paths
                      one behind another in path order
  new_names           rule 3: `_inv` behind a turned path's name (flip.py:27); the pool is the names one behind another
  candidates          rule 4: the link a -> b, overlap 0M, for every consecutive pair of a turned path's new steps, in path
                      order then step order (flip.py:43-68)
  dedup / dedup_fast  rule 5: the first link of every class, in order; two links are one class iff their overlaps are equal op
                      for op and they are the same (from, to) or each other's reverse complement (flip.py:33-40, gfa.py:190-194).
                      dedup is the reference's loop, quadratic; dedup_fast keys a set.
  check               rule 7: what is refused (IndexError where the library says FLATGFA_ERR_BOUNDS)

Every path is kept, also where several share a name: the reference keys its paths by name and would keep one.

Also here: the device code's geometry (flip_device.hpp), held against the source text by tests/test_flip_model.py.
"""
from __future__ import annotations

import os
import re
import tempfile
from typing import Dict, List, Tuple

import numpy as np

from oracle import flatgfa_oracle as fo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pollen_amd", "csrc")
THREADS, PER, GRID, SCAN_PER, SHORT_ROW, LDS_ROW = 256, 8, 2048, 4, 64, 4096
TILE = THREADS * PER
SCAN_TILE = THREADS * SCAN_PER
ZERO_M = 0  # one alignment op: length 0 above the low byte, opcode 0 (match)
SUFFIX = b"_inv"


def source_constants() -> Dict[str, int]:
    with open(os.path.join(CSRC, "flip_device.hpp")) as f:
        s = f.read()

    def one(pat):
        m = re.search(pat, s)
        assert m, pat
        return int(m.group(1))

    assert re.search(r"constexpr uint32_t kFlipTile = kFlipThreads \* kFlipPer;", s)
    return {"THREADS": one(r"constexpr int kFlipThreads = (\d+);"), "PER": one(r"constexpr uint32_t kFlipPer = (\d+);"),
            "GRID": one(r"constexpr uint32_t kFlipGrid = (\d+);"), "SCAN_PER": one(r"constexpr uint32_t kFlipScanPer = (\d+);"),
            "SHORT_ROW": one(r"constexpr uint32_t kFlipShortRow = (\d+);"), "LDS_ROW": one(r"constexpr uint32_t kFlipLdsRow = (\d+);")}


# ---- rule 7 ----
def check(p: fo.Pools) -> None:
    S = len(p.segs)
    a, b = p.segs["seq_start"].astype(np.int64), p.segs["seq_end"].astype(np.int64)
    if S and ((a > b).any() or (b > len(p.seq_data)).any()):
        raise IndexError("a segment's span leaves seq_data")
    a, b = p.paths["steps_start"].astype(np.int64), p.paths["steps_end"].astype(np.int64)
    if len(a) and ((a > b).any() or (b > len(p.steps)).any()):
        raise IndexError("a path's span leaves the steps")
    for s, e in zip(a, b):
        if ((p.steps[s:e] >> 1) >= S).any():
            raise IndexError("a step names no segment")
    if len(p.links):
        if ((p.links["from_"] >> 1) >= S).any() or ((p.links["to"] >> 1) >= S).any():
            raise IndexError("a link names no segment")
        if (p.links["ov_start"] > p.links["ov_end"]).any() or (p.links["ov_end"] > len(p.alignment)).any():
            raise IndexError("a link's overlap leaves the alignment pool")


def path_steps(p: fo.Pools, i: int) -> np.ndarray:
    return p.steps[int(p.paths["steps_start"][i]):int(p.paths["steps_end"][i])]


# ---- rule 1 ----
def weigh(p: fo.Pools, i: int) -> Tuple[int, int]:
    """(fwd, rev) of path i, as Python ints: no width to wrap."""
    st = path_steps(p, i)
    lens = (p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"].astype(np.int64))[st >> 1]
    back = (st & 1).astype(bool)
    return int(lens[~back].sum(dtype=np.uint64)), int(lens[back].sum(dtype=np.uint64))


def turned(p: fo.Pools) -> np.ndarray:
    out = np.zeros(len(p.paths), bool)
    for i in range(len(p.paths)):
        fwd, rev = weigh(p, i)
        out[i] = rev > fwd
    return out


# ---- rule 2 ----
def new_steps(p: fo.Pools, t: np.ndarray) -> List[np.ndarray]:
    return [(path_steps(p, i)[::-1] ^ np.uint32(1)) if t[i] else path_steps(p, i).copy() for i in range(len(p.paths))]


# ---- rule 3 ----
def new_names(p: fo.Pools, t: np.ndarray) -> List[bytes]:
    pool = p.name_data.tobytes()
    return [pool[int(r["name_start"]):int(r["name_end"])] + (SUFFIX if t[i] else b"") for i, r in enumerate(p.paths)]


# ---- rule 4 ----
def candidates(steps: List[np.ndarray], t: np.ndarray) -> List[Tuple[int, int]]:
    out: List[Tuple[int, int]] = []
    for i, st in enumerate(steps):
        if t[i]:
            out += [(int(a), int(b)) for a, b in zip(st[:-1], st[1:])]
    return out


# ---- rule 5 ----
Link = Tuple[int, int, Tuple[int, ...]]  # from, to, the overlap's ops


def rev(ln: Link) -> Link:
    return (ln[1] ^ 1, ln[0] ^ 1, ln[2])  # gfa.py:190-194


def dedup(links: List[Link]) -> List[int]:
    """flip.py:33-40: the indices kept."""
    new: List[Link] = []
    kept = []
    for k, item in enumerate(links):
        if item not in new and rev(item) not in new:
            new.append(item)
            kept.append(k)
    return kept


def dedup_fast(links: List[Link]) -> List[int]:
    seen = set()
    kept = []
    for k, item in enumerate(links):
        if item in seen or rev(item) in seen:
            continue
        seen.add(item)
        kept.append(k)
    return kept


def old_links(p: fo.Pools) -> List[Link]:
    al = p.alignment
    return [(int(r["from_"]), int(r["to"]), tuple(int(x) for x in al[int(r["ov_start"]):int(r["ov_end"])])) for r in p.links]


# ---- all of it ----
def flip(p: fo.Pools, fast: bool = True) -> fo.Pools:
    check(p)
    t = turned(p)
    steps = new_steps(p, t)
    names = new_names(p, t)
    cand = candidates(steps, t)
    old = old_links(p)
    kept = (dedup_fast if fast else dedup)(old + [(a, b, (ZERO_M,)) for a, b in cand])
    L, A = len(old), len(p.alignment)
    links = np.zeros(len(kept), fo.LINK_DT)
    for at, k in enumerate(kept):
        links[at] = p.links[k] if k < L else (cand[k - L][0], cand[k - L][1], A, A + 1)
    any_new = bool(kept) and kept[-1] >= L
    segs = np.zeros(len(p.segs), fo.SEG_DT)
    for f in ("name", "seq_start", "seq_end"):
        segs[f] = p.segs[f]
    paths = np.zeros(len(p.paths), fo.PATH_DT)
    n_end = np.cumsum([len(n) for n in names], dtype=np.int64) if names else np.zeros(0, np.int64)
    s_end = np.cumsum([len(s) for s in steps], dtype=np.int64) if steps else np.zeros(0, np.int64)
    if len(paths):
        paths["name_end"], paths["name_start"] = n_end, n_end - [len(n) for n in names]
        paths["steps_end"], paths["steps_start"] = s_end, s_end - [len(s) for s in steps]
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=p.header, segs=segs, paths=paths, links=links,
                    steps=np.concatenate(steps).astype(np.uint32) if steps else np.zeros(0, np.uint32), seq_data=p.seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT),
                    alignment=np.concatenate([p.alignment, np.array([ZERO_M], p.alignment.dtype)]) if any_new else p.alignment,
                    name_data=np.frombuffer(b"".join(names), np.uint8).copy(), optional_data=z, line_order=z)


def counts(p: fo.Pools) -> Tuple[int, int]:
    """(paths that turn, links of the result): what flip_count answers."""
    return int(turned(p).sum()), len(flip(p).links)


def row_sizes(p: fo.Pools) -> Dict[int, int]:
    """How many canonical keys -- of old links and candidates -- have each high handle: the rows of the device's key table."""
    t = turned(p)
    pairs = [(ln[0], ln[1]) for ln in old_links(p)] + candidates(new_steps(p, t), t)
    out: Dict[int, int] = {}
    for a, b in pairs:
        hi = min((a, b), (b ^ 1, a ^ 1))[0]
        out[hi] = out.get(hi, 0) + 1
    return out


# ---- helpers ----
def pools_of(g) -> fo.Pools:
    """The pools of a pollen_amd FlatGFA."""
    return fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})


def assert_same_pools(got: fo.Pools, want: fo.Pools, what="") -> None:
    for n in fo.POOL_ORDER:
        assert getattr(got, n).tobytes() == getattr(want, n).tobytes(), (n, what)


class handle_of:
    """A pollen_amd FlatGFA over these pools (through a .flatgfa file, which lives as long as the handle is used)."""

    def __init__(self, p: fo.Pools):
        self.p = p

    def __enter__(self):
        import pollen_amd as pa
        fd, self.path = tempfile.mkstemp(suffix=".flatgfa")
        with os.fdopen(fd, "wb") as f:
            f.write(fo.dump_flatgfa(self.p))
        self.g = pa.load(self.path)
        return self.g

    def __exit__(self, *exc):
        self.g.close()
        os.unlink(self.path)


def text(p: fo.Pools) -> bytes:
    """The GFA text the project's printer makes of these pools."""
    with handle_of(p) as g:
        return g.gfa_text()
