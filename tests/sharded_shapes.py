"""Graphs shaped around the packing, the cut rule and the grids of the sharded engine (pollen_amd/csrc/sharded.hip), for the
tests only.

  the packing   a cut path's touch counter is bits(n_shards) wide and 32 / bits of them share a u32: K cut paths take
                W = ceil(K / per_word) words per segment.  RINGS_MULTIWORD are the (paths, shards) pairs whose K passes
                one word; RING_SINGLE cuts ONE path into n_shards pieces that all touch every segment, so that the
                count is n_shards itself and needs the top bit of its field where n_shards is a power of two
  the grids     k_pack_touch and k_fix_uniq run min(ceil(S / 256), 2048) workgroups of 256 threads and stride from
                there: GRID_SEGS segments are one trip, `wide` has 300 more
  the cut rule  paths that do not lie in path order in the steps pool are never cut; CUT_LENGTHS are path lengths for
                the host-only cut function, some with totals beyond 2^56, where off * 8 * n_shards passes 2^64

Each factory returns a Shape: the graph, how to shard it and, for the planted shapes, the answer in closed form; want None:
tests/sharded_model.py's.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from oracle import flatgfa_oracle as fo
from sharded_model import Graph

GRID_SEGS = 2048 * 256  # one trip of k_pack_touch / k_fix_uniq
WIDE_SEGS = GRID_SEGS + 300
# (paths, shards, K, W): equal paths, one fewer than the shards -- the cut rule leaves the first and the last even cut at a
# path boundary (an eighth of a share is more than 1 / n_shards of a path there) and cuts the paths in between
RINGS_MULTIWORD = [(12, 13, 10, 2), (19, 20, 15, 3), (63, 64, 49, 13)]
RING_SINGLE = [2, 3, 4, 8, 16, 32, 64]
ERR_ARG, ERR_BOUNDS, ERR_TOO_LARGE = -1, -2, -6


class Shape(NamedTuple):
    name: str
    graph: Graph
    n_shards: int
    flags: int = 0
    depth: Optional[np.ndarray] = None  # uint64[S] in closed form; None: the model's
    uniq: Optional[np.ndarray] = None
    K: Optional[int] = None  # cut paths and packed words per segment, where the shape is built for them
    W: Optional[int] = None
    ordered: bool = True


def seg_lens(S: int) -> np.ndarray:
    return (1 + (np.arange(S, dtype=np.uint64) * 7 + 3) % 5).astype(np.uint32)


def pools(g: Graph) -> fo.Pools:
    """The graph as the eleven pools of a .flatgfa image (fo.dump_flatgfa writes them out): segments named 1 .. S with
    sequences of the given lengths, nameless paths with the given spans."""
    S, P = g.S, g.P
    ends = np.cumsum(g.seg_len.astype(np.uint64))
    segs = np.zeros(S, fo.SEG_DT)
    segs["name"] = np.arange(1, S + 1, dtype=np.uint64)
    segs["seq_end"] = ends.astype(np.uint32)
    segs["seq_start"] = (ends - g.seg_len).astype(np.uint32)
    paths = np.zeros(P, fo.PATH_DT)
    paths["steps_start"], paths["steps_end"] = g.begin, g.end
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=paths, links=np.zeros(0, fo.LINK_DT), steps=np.asarray(g.steps, np.uint32),
                    seq_data=np.full(int(ends[-1]) if S else 0, ord("A"), np.uint8), overlaps=np.zeros(0, fo.SPAN_DT),
                    alignment=np.zeros(0, np.uint32), name_data=z, optional_data=z,
                    line_order=np.concatenate([np.full(S, 1, np.uint8), np.full(P, 2, np.uint8)]))


def back_to_back(walks: List[np.ndarray], S: int) -> Graph:
    """Paths in path order in the steps pool, as the parser lays them out."""
    lens = np.array([len(w) for w in walks], np.int64)
    ends = np.cumsum(lens)
    steps = np.concatenate(walks).astype(np.uint32) if walks else np.zeros(0, np.uint32)
    return Graph(steps, ends - lens, ends, seg_lens(S))


# ---- ring paths: every piece touches every segment ----
def ring(P: int, L: int, S: int, n_shards: int, K: Optional[int] = None, W: Optional[int] = None) -> Shape:
    """P equal paths of L steps, step i on segment i % S (forward).  A piece of S steps or more touches every segment, so
    uniq == P and depth == P * L / S on every segment however the steps are cut."""
    assert L % S == 0
    walk = ((np.arange(L, dtype=np.uint32) % np.uint32(S)) << np.uint32(1))
    g = back_to_back([walk] * P, S)
    return Shape(f"ring-{P}x{L}-on-{n_shards}", g, n_shards, 0, np.full(S, P * L // S, np.uint64), np.full(S, P, np.uint64), K, W)


def ring_multiword(P: int, n_shards: int, K: int, W: int, S: int = 24) -> Shape:
    return ring(P, 40 * S, S, n_shards, K, W)


def ring_single(n_shards: int, S: int = 24) -> Shape:
    """ONE path on n_shards shards: n_shards pieces, and the count of every segment is n_shards."""
    return ring(1, 4 * S * n_shards, S, n_shards, 1 if n_shards > 1 else 0, 1 if n_shards > 1 else 0)


# ---- the same cuts, pieces that touch different subsets ----
def spokes(P: int, n_shards: int, K: Optional[int] = None, W: Optional[int] = None, L: int = 960) -> Shape:
    """P equal paths of L steps over S = 2 L + 3 P segments.  Path p walks an arc of its own (every other step; offset 37 p,
    downwards and on backward handles for odd p): a segment of it belongs to one piece.  Every fifth step is on the path's
    hub, which every piece touches, every seventh step of the first half on its half hub, and every third step of the last
    third on a segment that the next path's arc crosses too.  A cut path's count thus runs from 0 to its number of pieces
    over the segments.  The answer is the model's."""
    S = 2 * L + 3 * P
    i = np.arange(L, dtype=np.int64)
    walks = []
    for p in range(P):
        off, sign = 37 * p, (-1 if p & 1 else 1)
        seg = (off + sign * (i // 2)) % (2 * L)
        seg = np.where(i % 5 == 0, 2 * L + 3 * p, seg)
        seg = np.where((i % 7 == 0) & (i < L // 2), 2 * L + 3 * p + 1, seg)
        seg = np.where((i % 3 == 1) & (i >= 2 * L // 3), (37 * (p + 1) + 5) % (2 * L), seg)
        walks.append(((seg << 1) | ((i + p) & 1 if p % 3 else p & 1)).astype(np.uint32))
    return Shape(f"spokes-{P}-on-{n_shards}", back_to_back(walks, S), n_shards, 0, None, None, K, W)


# ---- more segments than one trip of the fix-up grids ----
def wide(S: int = WIDE_SEGS, n_shards: int = 4) -> Shape:
    """Three paths that each walk 0 .. S-1 twice, on four shards: the even cuts lie at 1.5 S, 3 S and 4.5 S steps, half a
    path from any boundary, so every path is cut in two: path 1 between its laps, path 0 half a lap before its end, path 2
    half a lap in.  Every segment is touched by both pieces of path 1 and of one other path, so uniq would be 5 without the
    fix-up."""
    assert S % 2 == 0
    lap = np.arange(S, dtype=np.uint32) << np.uint32(1)
    g = back_to_back([np.concatenate([lap, lap])] * 3, S)
    return Shape(f"wide-{S}", g, n_shards, 0, np.full(S, 6, np.uint64), np.full(S, 3, np.uint64), 3, 1)


# ---- paths that do not lie in path order in the steps pool ----
def _walks(rng, P: int, S: int, lo: int, hi: int) -> List[np.ndarray]:
    return [rng.integers(0, 2 * S, int(rng.integers(lo, hi))).astype(np.uint32) for _ in range(P)]


def out_of_order(kind: str, n_shards: int = 5, seed: int = 7) -> Shape:
    """`reversed`: path p's steps lie behind those of path p + 1.  `interleaved`: the pool holds the paths in the order 0, 2,
    1, 3, ...  `shared`: two paths walk overlapping stretches of the pool, a third one a stretch inside another's.  `empties`:
    reversed, with empty paths (spans 0..0, N..N and one in the middle) at the start, in between and at the end.
    `ordered-empties` is in pool order -- and so may be cut -- with empty paths at the start, at the end and where the even
    cuts fall."""
    rng = np.random.default_rng(seed)
    S = 300
    if kind == "ordered-empties":
        w = _walks(rng, 4, S, 500, 501)
        z = np.zeros(0, np.uint32)
        g = back_to_back([z, w[0], z, z, w[1], z, w[2], z, w[3], z, z], S)
        return Shape(kind, g, n_shards, 0)
    w = _walks(rng, 7, S, 40, 400)
    lens = [len(x) for x in w]
    if kind == "shared":
        steps = rng.integers(0, 2 * S, 1500).astype(np.uint32)
        b = np.array([0, 300, 350, 900, 100], np.int64)
        e = np.array([500, 800, 450, 1500, 100], np.int64)
        return Shape(kind, Graph(steps, b, e, seg_lens(S)), n_shards, 0, ordered=False)
    order = {"reversed": list(range(6, -1, -1)), "interleaved": [0, 2, 1, 3, 5, 4, 6], "empties": list(range(6, -1, -1))}[kind]
    pos, at = {}, 3  # (three steps of no path in front, and two between the paths)
    for p in order:
        pos[p] = at
        at += lens[p] + 2
    steps = rng.integers(0, 2 * S, at).astype(np.uint32)
    for p in range(7):
        steps[pos[p]:pos[p] + lens[p]] = w[p]
    b = [pos[p] for p in range(7)]
    e = [pos[p] + lens[p] for p in range(7)]
    if kind == "empties":
        mid = pos[3] + 5
        b = [0] + b[:3] + [mid, mid] + b[3:] + [at]
        e = [0] + e[:3] + [mid, mid] + e[3:] + [at]
    return Shape(kind, Graph(steps, np.array(b, np.int64), np.array(e, np.int64), seg_lens(S)), n_shards, 0, ordered=False)


OUT_OF_ORDER = ["reversed", "interleaved", "shared", "empties", "ordered-empties"]


# ---- path lengths for the host-only cut function ----
def cut_lengths() -> List[Tuple[str, List[int], int]]:
    """(name, path lengths, n_shards).  The `huge` ones have totals from 2^56 on, where the distance of a path boundary from
    the even cut, times 8 n_shards, no longer fits 64 bits; every total stays below 2^64."""
    out = []
    for n in (1, 2, 3, 8, 13, 64):
        out.append((f"equal-{n}", [1000] * 12, n))
        out.append((f"giant-{n}", [50, 900, 70] + [10 ** 6] + [30] * 20, n))
        out.append((f"all-empty-{n}", [0] * 9, n))
        out.append((f"no-paths-{n}", [], n))
        out.append((f"empties-at-cuts-{n}", [0, 500, 0, 0, 500, 0, 500, 0, 500, 0, 0], n))
    out.append(("huge-one-path-3", [1 << 61], 3))  # (the cut at 2 T / 3 is T / 3 from the end: times 24 that is 2^64 and more)
    out.append(("huge-one-path-64", [1 << 56], 64))  # (the least total that wraps with 64 shards)
    out.append(("huge-below-wrap-64", [(1 << 56) - 64], 64))
    out.append(("huge-seven-paths-5", [1 << 61] * 7, 5))
    out.append(("huge-giant-among-short-7", [5, 1 << 40, (1 << 63) + 12345, 3, 1 << 62, 0, 9], 7))
    out.append(("huge-uneven-64", [(1 << 58) + 3 * k for k in range(60)], 64))
    out.append(("huge-near-boundaries-3", [(1 << 61) + 1, (1 << 61) - 5, 1 << 61], 3))
    return out
