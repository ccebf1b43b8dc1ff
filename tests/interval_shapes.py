"""Small graphs and interval lists for interval depth over many paths (tests/test_interval_model.py on the model,
tests/test_gpu_interval_depth.py on the GPU).  Every shape is a set of pools plus named lists (path ids, starts, ends), one
list per call; a shape has at most a few thousand steps, `tiles` about nine thousand (six paths around one and two scan tiles
of 1024 steps, which is what interval_device.hip's kThreads * kPer comes to).

What the lists cover, on every path that has the room: ends on step seams, one base either side of a seam, inside one step;
the whole path and past it; 63, 64, 65, 128 and 129 steps (the wave rounds' edges) from a seam and from inside a step; the
last step only; start == end, start > end, start at and beyond the path's length; steps of no length inside, at the start
and at the end of an interval; a path with no steps; sorted-disjoint, sorted-overlapping, unsorted and nested lists (where
M drops terms); A,B,A with one interval per group; more groups of long intervals than k_long has waves; spans that overlap
and leave gaps in the steps pool; positions beyond 2^32.  budget_cases() lowers the batch budget, for the stand-alone program.

Test infrastructure only."""
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

import chop_shapes
from oracle import flatgfa_oracle as fo

TILE = 1024        # kThreads * kPer of interval_device.hip
LONG_WAVES = 4096  # kLongGrid * 4: the waves of one k_long launch
LANE_CUT = 8        # kIntervalLaneCut


@dataclass
class Shape:
    name: str
    pools: fo.Pools
    lists: Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray]] = field(default_factory=dict)

    def add(self, label, ids, starts, ends):
        assert label not in self.lists, label
        ids = np.asarray(ids, np.uint32)
        starts, ends = np.asarray(starts, np.uint64), np.asarray(ends, np.uint64)
        if ids.ndim == 0:
            ids = np.full(len(starts), int(ids), np.uint32)
        assert len(ids) == len(starts) == len(ends)
        self.lists[label] = (ids, starts, ends)


def make_pools(lens, steps, spans) -> fo.Pools:
    """Segments whose sequence spans alias one pool of max(lens) bases (flatgfa_load checks that a span lies inside its pool,
    not that spans are disjoint); paths named p0, p1, ..."""
    lens = np.asarray(lens, np.int64)
    p = chop_shapes.make_pools(lens, steps, spans, seq=False)
    p.seq_data = np.full(int(lens.max()) if len(lens) else 0, ord("A"), np.uint8)
    names = [b"p%d" % k for k in range(len(p.paths))]
    at = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.int64)
    p.paths["name_start"], p.paths["name_end"] = at[:-1], at[1:]
    p.name_data = np.frombuffer(b"".join(names), np.uint8).copy()
    return p


def ends_of(pools, pid) -> List[int]:
    p = pools.paths[pid]
    segs = pools.steps[int(p["steps_start"]):int(p["steps_end"])].astype(np.int64) >> 1
    return [int(x) for x in np.cumsum(pools.seg_lens()[segs].astype(np.uint64))]


def edge_lists(s: Shape, pid: int, rng, tag: str) -> None:
    """The lists every path gets."""
    r1 = ends_of(s.pools, pid)
    L = r1[-1] if r1 else 0
    r0 = [0] + r1[:-1]
    n = len(r1)
    st, en = [], []
    for j in sorted({int(x) for x in rng.integers(0, n, 12)} | {0, n - 1}) if n else []:
        st += [r0[j], max(r0[j], 1) - 1, r0[j] + 1, r0[j]]
        en += [r1[j], r1[j] + 1, max(r1[j], 1) - 1, r0[j] + 1]  # (the third is inverted or empty on a short step)
    s.add(tag + "seams", pid, st, en)
    s.add(tag + "whole", pid, [0, 0, 1, 0], [L, L + 10, L + 1, max(L, 1) - 1])
    s.add(tag + "degenerate", pid, [5, 9, L, L + 7, 0, L, 2 ** 64 - 1, 3], [5, 2, L + 3, L + 9, 0, L, 2 ** 64 - 1, 0])
    if n:
        s.add(tag + "last", pid, [r0[-1], r0[-1], max(L, 1) - 1], [L, L + 5, L])
    st, en = [], []
    for k in (63, 64, 65, 128, 129):
        for a in (0, 7):
            if a + k <= n:
                st += [r0[a], r0[a] + (1 if r1[a] - r0[a] > 1 else 0)]
                en += [r1[a + k - 1], r1[a + k - 1]]
    if st:
        s.add(tag + "rounds", pid, st, en)
    if L > 4:
        cuts = np.unique(np.concatenate([[0, L], rng.integers(1, L, 40)]))
        s.add(tag + "sorted_disjoint", pid, cuts[:-1], cuts[1:])
        a = np.sort(rng.integers(0, L, 60))
        s.add(tag + "sorted_overlapping", pid, a, a + rng.integers(0, max(L // 3, 2), 60))
        a = rng.integers(0, L + 3, 80)
        s.add(tag + "unsorted", pid, a, np.maximum(a + rng.integers(-3, max(L // 2, 2), 80), 0))
        q = L // 8
        s.add(tag + "nested", pid, [0, q, 2 * q, q + 1, 5 * q, 3 * q, 0, 7 * q, 6 * q, 2], [L, 2 * q, 3 * q, 6 * q, 6 * q, 4 * q, L, L, L + 1, 3])


def basic() -> Shape:
    """Four paths whose spans overlap and leave gaps in the steps pool; lengths 0..9, one segment in five of no length; one
    path without steps."""
    rng = np.random.default_rng(11)
    S = 60
    lens = rng.integers(1, 10, S)
    lens[rng.integers(0, S, S // 5)] = 0
    steps = chop_shapes.handles(rng, rng.integers(0, S, 700))
    s = Shape("basic", make_pools(lens, steps, [(3, 303), (250, 450), (460, 460), (500, 630)]))
    for pid in range(4):
        edge_lists(s, pid, rng, "p%d_" % pid)
    L = [(ends_of(s.pools, p) or [0])[-1] for p in range(4)]
    s.add("aba", [0, 1, 0], [10, 10, 12], [L[0] - 3, L[1] - 3, L[0]])
    s.add("empty_path_between", [0, 2, 2, 3, 2, 1], [0, 0, 5, 0, 1, 4], [50, 50, 9, L[3], 0, L[1] + 4])
    ids = rng.integers(0, 4, 300)
    a = rng.integers(0, max(L) + 5, 300)
    s.add("mixed_groups", ids, a, a + rng.integers(0, 400, 300))
    ids = np.repeat(rng.integers(0, 4, 40), rng.integers(1, 9, 40))
    a = rng.integers(0, max(L), len(ids))
    s.add("runs", ids, a, a + rng.integers(0, 300, len(ids)))
    return s


def zeros() -> Shape:
    """Steps of no length at the start, inside and at the end of the path and of the intervals."""
    lens = [0, 3, 4, 2, 0, 5]
    segs = [0, 4, 1, 0, 2, 4, 0, 3, 0, 4, 5, 0, 4]  # 0 0 3 0 4 0 0 2 0 0 5 0 0: ends 0 0 3 3 7 7 7 9 9 9 14 14 14
    only0 = [0, 4, 0]
    steps = np.array([x << 1 for x in segs + only0], np.uint32)
    s = Shape("zeros", make_pools(lens, steps, [(0, len(segs)), (len(segs), len(segs) + 3)]))
    s.add("grid", 0, [a for a in range(0, 16) for b in range(0, 17)], [b for a in range(0, 16) for b in range(0, 17)])
    s.add("windows1", 0, list(range(14)), list(range(1, 15)))
    s.add("no_bases", 1, [0, 0, 1, 0], [1, 0, 2, 5])
    return s


def tiles() -> Shape:
    """Step counts around one and two scan tiles; the batch's scan restarts at every path, wherever in a tile that falls."""
    rng = np.random.default_rng(12)
    S = 200
    lens = rng.integers(0, 7, S)
    counts = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
    spans, at = [], 2
    for c in counts:
        spans.append((at, at + c))
        at += c + int(rng.integers(0, 4))
    steps = chop_shapes.handles(rng, rng.integers(0, S, at + 2))
    s = Shape("tiles", make_pools(lens, steps, spans))
    ids, st, en = [], [], []
    for pid in (3, 0, 5, 1, 4, 2):
        r1 = ends_of(s.pools, pid)
        L = r1[-1]
        w = [(a, min(a + 100, L)) for a in range(0, L, 100)]
        rows = [(0, L), (r1[-2], L), (r1[TILE - 3], r1[TILE - 2] + 1)] + w
        ids += [pid] * len(rows)
        st += [r[0] for r in rows]
        en += [r[1] for r in rows]
    s.add("all_paths", ids, st, en)
    s.add("one_path", 4, st[:40], en[:40])
    return s


def many_groups() -> Shape:
    """More groups of one long interval each than one k_long launch has waves."""
    rng = np.random.default_rng(13)
    S = 30
    lens = rng.integers(1, 6, S)
    steps = chop_shapes.handles(rng, rng.integers(0, S, 260))
    s = Shape("many_groups", make_pools(lens, steps, [(0, 120), (100, 260)]))
    n = LONG_WAVES + 150
    ids = np.arange(n) & 1
    r = [ends_of(s.pools, 0), ends_of(s.pools, 1)]
    first = rng.integers(0, 40, n)
    count = rng.integers(LANE_CUT + 1, 75, n)
    st = [r[p][a] - 1 for p, a in zip(ids, first)]
    en = [r[p][a + c] for p, a, c in zip(ids, first, count)]
    s.add("alternating", ids, st, en)
    return s


def long_positions() -> Shape:
    """Positions beyond 2^32: a few segments of 2^22 bases, walked a few thousand times."""
    rng = np.random.default_rng(14)
    lens = np.array([1 << 22, 3, (1 << 22) - 5, 0, 17, 1 << 21], np.int64)
    segs = rng.choice([0, 0, 2, 2, 0, 2, 5, 1, 3, 4], 3000)
    steps = chop_shapes.handles(rng, segs)
    s = Shape("long_positions", make_pools(lens, steps, [(0, 3000), (300, 2800)]))
    for pid in range(2):
        r1 = ends_of(s.pools, pid)
        L = r1[-1]
        assert L > (1 << 32) + (1 << 30)
        j = next(k for k, e in enumerate(r1) if e > 1 << 32)
        st = [0, (1 << 32) - 1, 1 << 32, r1[j - 1], r1[j - 1] - 1, (1 << 32) - 100, r1[-2], 1 << 31]
        en = [L, (1 << 32) + 1, (1 << 32) + 1, r1[j], r1[j + 70], (1 << 32) + 100, L, (1 << 33)]
        s.add("p%d_edges" % pid, pid, st, en)
        w = 1 << 28
        s.add("p%d_windows" % pid, pid, list(range(0, L, w)), [min(a + w, L) for a in range(0, L, w)])
        a = rng.integers(0, L, 50)
        s.add("p%d_unsorted" % pid, pid, a, a + rng.integers(0, 1 << 31, 50))
    return s


SHAPES = [basic, zeros, tiles, many_groups, long_positions]


@functools.lru_cache(maxsize=None)
def shape(name: str) -> Shape:
    return {f.__name__: f for f in SHAPES}[name]()


def budget_cases():
    """(label, list of path ids, budget, batches): the groups of `basic` (300, 200, 0 and 130 steps) against a lowered budget.
    500: the cut falls between two groups (0 1 | 3 ...); 300: a path is in two batches, and the cut falls between two of
    its groups (0 | 1 | 0 ...); 1: every group that names a new path starts a batch."""
    return [
        ("fits", [0, 1, 0, 3, 2, 1], 1 << 27, 1),
        ("between_groups", [0, 1, 0, 3, 2, 1, 3], 500, 2),   # {0 1} 0 | {3 2 1} 3
        ("same_path", [0, 1, 0, 2, 0, 3, 1], 300, 5),         # {0} | {1} | {0 2} 0 | {3} | {1}
        ("every_group", [0, 1, 0, 3, 3, 1, 2, 2, 0], 1, 7),   # {0} | {1} | {0} | {3} 3 | {1} | {2} 2 | {0}
    ]


def budget_list(label: str, groups, seed: int):
    """Five intervals per group of `basic`, unsorted."""
    s = shape("basic")
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.asarray(groups, np.uint32), 5)
    L = np.array([(ends_of(s.pools, p) or [0])[-1] for p in range(4)])[ids]
    a = rng.integers(0, L + 2)
    return ids, a.astype(np.uint64), (a + rng.integers(0, 500, len(ids))).astype(np.uint64)


def plan_batches(groups, lengths, budget) -> int:
    """How many batches the plan makes of these groups (plan_interval_batches in flatgfa_core.cpp, restated)."""
    batches, held, steps = 1, set(), 0
    for k, p in enumerate(groups):
        if k and groups[k - 1] == p:
            continue
        if p in held:
            continue
        if held and steps + lengths[p] > budget:
            batches, held, steps = batches + 1, set(), 0
        held.add(p)
        steps += lengths[p]
    return batches
