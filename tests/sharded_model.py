"""An exact CPU model of the sharded engine (pollen_amd/csrc/sharded.hip, the flatgfa_sharded_* entries of
include/flatgfa.h), for the tests only: numpy and Python integers, written from DESIGN.md section 6 and the header.

  cuts       where the path steps are cut: cut r is the path boundary nearest the even cut T * r / n (ties: the lower
             one) when paths stay whole or when that boundary lies within an eighth of a shard's share of the even cut
             (|boundary - even| * 8 * n <= T), the even cut itself otherwise; never before the cut to its left
  layout     per shard the pieces (path, first step, last step) it walks, the stretch of the steps pool that covers
             them, the first path it has steps of; per handle the cut paths in path order (their split ordinals), the
             counter width bits(n), counters per word, words per segment and the bytes of the collective.  A graph
             whose paths do not lie in path order in the steps pool is never cut inside a path
  exchange   every shard's [depth | uniq | packed touch] vector, their sum in u32, the fix-up of unique depth
  path_depth per piece the two integer sums of measure_path, added per path, one float64 division

Everything is a sum of small integers: there is nothing to round, and the model says so by asserting that no counter
field of the summed vector passes n_shards and that n_shards fits a field.
"""
from __future__ import annotations

import bisect
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

WHOLE_PATHS = 1  # FLATGFA_SHARD_WHOLE_PATHS
MAX_SHARDS = 64


class Graph(NamedTuple):
    steps: np.ndarray  # uint32 handles: segment << 1 | backward
    begin: np.ndarray  # [P] every path's span of the steps pool
    end: np.ndarray
    seg_len: np.ndarray  # uint32[S]

    @property
    def S(self) -> int:
        return len(self.seg_len)

    @property
    def P(self) -> int:
        return len(self.begin)


def graph_of(pools) -> Graph:
    """An oracle Pools object as the model's graph."""
    return Graph(np.asarray(pools.steps, np.uint32), np.asarray(pools.paths["steps_start"], np.int64),
                 np.asarray(pools.paths["steps_end"], np.int64), pools.seg_lens())


def cuts(path_steps: Sequence[int], n_shards: int, whole_paths: bool = False) -> List[int]:
    """n_shards + 1 cut points, counted in path steps along the path order (Python integers: nothing can wrap)."""
    assert 1 <= n_shards <= MAX_SHARDS
    ends = [0]
    for x in path_steps:
        ends.append(ends[-1] + int(x))
    T = ends[-1]
    out = [0]
    for r in range(1, n_shards):
        even = T * r // n_shards
        i = bisect.bisect_right(ends, even)  # ends[i - 1] <= even < ends[i]
        below = ends[i - 1]
        above = ends[i] if i < len(ends) else below
        near = below if even - below <= above - even else above
        c = near if whole_paths or abs(near - even) * 8 * n_shards <= T else even
        out.append(max(c, out[-1]))
    out.append(T)
    return out


class ShardLayout(NamedTuple):
    pieces: Tuple[Tuple[int, int, int], ...]  # (path, first step, one past its last step), positions in the steps pool
    step_begin: int  # the stretch of the pool that covers the pieces ((0, 0): none)
    step_end: int
    first_path: int  # P: the shard walks nothing


class Layout(NamedTuple):
    n_shards: int
    S: int
    P: int
    ordered: bool
    cuts: Tuple[int, ...]
    shards: Tuple[ShardLayout, ...]
    split_paths: Tuple[int, ...]  # the cut paths; the index is the path's split ordinal
    bits: int
    per_word: int
    W: int

    @property
    def K(self) -> int:
        return len(self.split_paths)

    def split_of(self, path: int) -> int:
        return self.split_paths.index(path) if path in self.split_paths else -1

    def collective_bytes(self, with_uniq: bool) -> int:
        return 4 * self.S * (2 + self.W if with_uniq else 1)


def layout(g: Graph, n_shards: int, flags: int = 0) -> Layout:
    P = g.P
    b = [int(x) for x in g.begin]
    e = [int(x) for x in g.end]
    assert all(x <= y <= len(g.steps) for x, y in zip(b, e))
    ordered = all(b[p] >= e[p - 1] for p in range(1, P))
    cut = cuts([y - x for x, y in zip(b, e)], n_shards, whole_paths=bool(flags & WHOLE_PATHS) or not ordered)
    ends = [0]
    for x, y in zip(b, e):
        ends.append(ends[-1] + (y - x))
    shards, split = [], set()
    for r in range(n_shards):
        lo, hi = cut[r], cut[r + 1]
        pieces = []
        for p in range(P):
            x, y = max(ends[p], lo), min(ends[p + 1], hi)
            if x >= y:
                continue
            pieces.append((p, b[p] + (x - ends[p]), b[p] + (y - ends[p])))
            if (x, y) != (ends[p], ends[p + 1]):
                split.add(p)
        if pieces:
            shards.append(ShardLayout(tuple(pieces), min(x[1] for x in pieces), max(x[2] for x in pieces), pieces[0][0]))
        else:
            shards.append(ShardLayout((), 0, 0, P))
    bits = n_shards.bit_length()  # the least width that holds n_shards itself: a path cut into n_shards pieces counts that far
    per_word = 32 // bits
    K = len(split)
    return Layout(n_shards, g.S, P, ordered, tuple(cut), tuple(shards), tuple(sorted(split)), bits, per_word, -(-K // per_word))


def _piece_counts(g: Graph, piece) -> np.ndarray:
    _, x, y = piece
    ids = (g.steps[x:y] >> 1).astype(np.int64)
    assert not len(ids) or int(ids.max()) < g.S, "a step names a segment that is not there"
    return np.bincount(ids, minlength=g.S)


def shard_vectors(g: Graph, lay: Layout) -> List[np.ndarray]:
    """What every shard sends: uint32[(2 + W) * S], [depth | uniq | W words of packed touch counters per segment]; a piece
    counts as a path of its own, and a piece of split path k adds one to field k % per_word of word k // per_word."""
    S = g.S
    out = []
    for sh in lay.shards:
        v = np.zeros((2 + lay.W, S), np.uint32)
        for piece in sh.pieces:
            n = _piece_counts(g, piece)
            v[0] += n.astype(np.uint32)
            v[1] += (n > 0).astype(np.uint32)
            k = lay.split_of(piece[0])
            if k >= 0:
                v[2 + k // lay.per_word] += (n > 0).astype(np.uint32) << np.uint32((k % lay.per_word) * lay.bits)
        out.append(v.reshape(-1))
    return out


def fields(lay: Layout, packed: np.ndarray) -> np.ndarray:
    """The K counters of every segment, int64[K, S], out of the summed packed words uint32[W, S]."""
    mask = (1 << lay.bits) - 1
    out = np.zeros((lay.K, lay.S), np.int64)
    for k in range(lay.K):
        out[k] = (packed[k // lay.per_word].astype(np.int64) >> ((k % lay.per_word) * lay.bits)) & mask
    return out


def exchange(g: Graph, lay: Layout):
    """The reduced (depth, uniq) as uint64[S], and the summed packed words uint32[W, S]."""
    S = g.S
    assert lay.n_shards < 2 ** lay.bits
    total = np.zeros((2 + lay.W) * S, np.uint32)
    for v in shard_vectors(g, lay):
        total = total + v  # u32, as the collective adds
    total = total.reshape(2 + lay.W, S)
    depth, uniq, packed = total[0].astype(np.int64), total[1].astype(np.int64), total[2:]
    m = fields(lay, packed)
    # a field is the number of pieces of one path that touch the segment; counted piece by piece it must come out the same
    pieces_of = {k: 0 for k in range(lay.K)}
    direct = np.zeros((lay.K, S), np.int64)
    for sh in lay.shards:
        for piece in sh.pieces:
            k = lay.split_of(piece[0])
            if k >= 0:
                pieces_of[k] += 1
                direct[k] += _piece_counts(g, piece) > 0
    assert (m == direct).all(), "a counter ran into its neighbour"
    assert not lay.K or int(m.max()) <= lay.n_shards
    assert all(n <= lay.n_shards for n in pieces_of.values())
    uniq = uniq - np.maximum(m - 1, 0).sum(axis=0)
    assert (uniq >= 0).all()
    return depth.astype(np.uint64), uniq.astype(np.uint64), packed


def path_depth(g: Graph, lay: Layout, depth: np.ndarray = None) -> Tuple[np.ndarray, np.ndarray]:
    """(lengths uint64[P], mean depths float64[P]): per piece the sum of the segment lengths and the sum of depth times
    length over its steps, the pieces of a path added up, one division (0 / 0: NaN, as the reference prints it)."""
    if depth is None:
        depth = exchange(g, lay)[0]
    ln = [0] * g.P
    ws = [0] * g.P
    sl = g.seg_len.astype(np.uint64)
    for sh in lay.shards:
        for p, x, y in sh.pieces:
            ids = (g.steps[x:y] >> 1).astype(np.int64)
            ln[p] += int(sl[ids].sum(dtype=np.uint64))
            ws[p] += int((sl[ids] * depth[ids].astype(np.uint64)).sum(dtype=np.uint64))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.array(ws, np.uint64).astype(np.float64) / np.array(ln, np.uint64).astype(np.float64)
    return np.array(ln, np.uint64), mean
