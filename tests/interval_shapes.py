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

And at the seams of what the kernels tile over: long_groups (one group across the max-scan's tiles, k_spine's second round and
k_intervals' stride; heads on the tile seams), many_paths (three thousand slots, runs of stepless paths on a tile seam and at
a batch's ends), cut_edges (7, 8 and 9 walked steps; paths of 64 and 128), big_products (u64 -> f64 rounding; raw arrays).

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
    seams: Dict[str, List[int]] = field(default_factory=dict)  # per list: indices inside a group that M must be carried across
    heads: Dict[str, List[int]] = field(default_factory=dict)  # per list: group heads at which M must restart
    notes: Dict[str, object] = field(default_factory=dict)    # what a shape's tests need to know of its geometry

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


SPINE_ROUND = 256 * TILE    # k_spine takes 256 tile aggregates a round: its second round begins at this interval
STRIDE = 2048 * 256         # kMaxGrid * kThreads: k_intervals strides over the intervals from here upwards
WIDE = 1 << 24


def step_ends_within(r1, a, b) -> int:
    """How many steps end in (a, b]."""
    return int(np.searchsorted(r1, b, "right") - np.searchsorted(r1, a, "right"))


def ascending(L: int, n: int):
    """n windows of width L // n + 3, window i from i * (L // n): sorted, each reaching 3 bases into the next, so M is the end
    of the window before and drops next to nothing.  (Unsorted random lists come out almost all 0.0 in long groups: the cursor
    is past them.)"""
    g = L // n
    st = np.arange(n, dtype=np.uint64) * np.uint64(g)
    return st, st + np.uint64(g + 3)


def long_groups() -> Shape:
    """Groups of thousands of intervals on the pools of long_positions: M carried across the max-scan's tile seams, through
    k_spine and into its second round, across k_intervals' stride; M restarting at heads on and around the tile seams; a
    tile whose own ends all lie below the M it must hand on."""
    lp = long_positions()
    s = Shape("long_groups", lp.pools)
    r1 = [np.array(ends_of(s.pools, p), np.uint64) for p in range(2)]
    L = [int(r[-1]) for r in r1]
    assert min(L) > 1 << 32

    def carried(label, n, seams, step_ends=3):
        st, en = ascending(L[0], n)
        assert n > max(seams) + 2 and int(en[-1]) <= L[0] + 3
        for q in seams:  # the interval two before the seam reaches far past the ones behind the seam
            a = int(st[q - 2])
            en[q - 2] = a + WIDE
            assert (q - 2) // TILE == q // TILE - 1 and q % TILE == 0
            assert step_ends_within(r1[0], a, a + WIDE) >= step_ends
            assert step_ends == 3 or (a + WIDE > L[0] and step_ends_within(r1[0], a, L[0]) == step_ends)
            assert int(en[q + 1]) < a + WIDE  # (the seam's interval and the one behind it end below that M)
        s.add(label, 0, st, en)
        s.seams[label] = list(seams)

    carried("tile_seams", 3 * TILE + 5, [TILE, 2 * TILE, 3 * TILE])
    carried("spine_round", SPINE_ROUND + TILE + 3, [SPINE_ROUND])
    # (257 windows from the path's end only two steps are left to end, 2^24 bases reach past the path, and that M drops every
    # term of every interval behind the seam)
    carried("stride", STRIDE + 257, [STRIDE], step_ends=2)

    # heads on and around the tile seams: the group in front of each ends on an interval that reaches its path's end
    heads = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE]
    n = 2 * TILE + 100
    ids = np.zeros(n, np.uint32)
    for k, h in enumerate(heads):
        ids[h:] = (k + 1) & 1
    st, en = ascending(min(L), n)
    for h in heads:
        en[h - 1] = L[int(ids[h - 1])]
        assert ids[h] != ids[h - 1] and int(st[h - 1]) < L[int(ids[h - 1])]
    s.add("heads", ids, st, en)
    s.heads["heads"] = heads

    # tile 1's ends all lie below the M that tile 0 sets; tile 2 begins below it and leaves it
    n = 3 * TILE + 7
    st, en = ascending(L[0], n)
    big = int(st[2 * TILE + 20]) + 5
    en[TILE - 24] = big
    assert int(en[TILE:2 * TILE].max()) < big and int(en[:TILE - 24].max()) < big
    assert int(en[2 * TILE]) < big < int(st[2 * TILE + 40])
    assert step_ends_within(r1[0], int(st[2 * TILE]), big) >= 3
    s.add("through_a_tile", 0, st, en)
    s.seams["through_a_tile"] = [2 * TILE]
    return s


def many_paths() -> Shape:
    """About 3000 paths of 0 to 5 steps over segments of 0 to 6 bases; the list names them in a shuffled order, which is the
    batch's slot order.  In that order: three stepless paths at the front, three at the end, three where the batch's step 1024
    lies (so one path ends at 1024 and one starts there), and one stepless path between a path that ends at step 2048 and one
    that starts there."""
    rng = np.random.default_rng(21)
    S = 40
    lens = rng.integers(0, 7, S)
    lens[:6] = [0, 0, 3, 6, 1, 0]
    counts = [0, 0, 0, 3]

    def fill_to(total):
        while sum(counts) < total:
            c = min(int(rng.integers(0, 6)), total - sum(counts))
            if sum(counts) + c == total and c < 2:  # the path that ends there has two steps or more
                counts.append(0)
                continue
            if 0 < total - sum(counts) - c < 2:
                c -= 1
            counts.append(c)

    fill_to(TILE)
    at_tile = len(counts)
    counts.extend([0, 0, 0, 4])
    fill_to(2 * TILE)
    at_two = len(counts)
    counts.extend([0, 2])
    while len(counts) < 2990:
        counts.append(int(rng.integers(0, 6)))
    counts.extend([5, 0, 0, 0])
    counts = np.array(counts)
    P = len(counts)
    order = rng.permutation(P)           # slot k holds path order[k]
    per_path = np.zeros(P, np.int64)
    per_path[order] = counts
    begin = np.concatenate([[0], np.cumsum(per_path)])
    steps = chop_shapes.handles(rng, rng.integers(0, S, int(begin[-1])))
    s = Shape("many_paths", make_pools(lens, steps, np.stack([begin[:-1], begin[1:]], axis=1)))
    # ---- the geometry, in slot order ----
    pstart = np.concatenate([[0], np.cumsum(counts)])
    assert (lens == 0).any() and 2900 < P < 3100 and counts.max() == 5 and counts.min() == 0
    assert (counts[:3] == 0).all() and counts[3] > 0 and (counts[-3:] == 0).all() and counts[-4] >= 2
    assert pstart[at_tile] == TILE and (counts[at_tile:at_tile + 3] == 0).all() and counts[at_tile - 1] >= 2 and counts[at_tile + 3] > 0
    assert pstart[at_two] == 2 * TILE and counts[at_two] == 0 and counts[at_two - 1] >= 2 and counts[at_two + 1] > 0
    assert pstart[-1] > 7 * TILE
    s.notes.update(order=order, counts=counts, at_tile=at_tile, at_two=at_two)

    def listed(slots, whole_first=False):
        ids, st, en = [], [], []
        for k in slots:
            L = (ends_of(s.pools, int(order[k])) or [0])[-1]
            w = [(a, min(a + 3, L)) for a in range(0, L, 3)]
            # (behind its windows M leaves the whole path its last steps only; in front of them it would leave them nothing)
            rows = [(0, L), (L, L + 4)] if whole_first else w + [(0, L), (L, L + 4)]
            ids += [int(order[k])] * len(rows)
            st += [r[0] for r in rows]
            en += [r[1] for r in rows]
        return ids, st, en

    s.add("slot_order", *listed(range(P)))
    # every path again, backwards, its whole length first in its group: groups on paths the batch already holds
    there, back = listed(range(P)), listed(range(P - 2, -1, -1), True)
    s.add("there_and_back", *[a + b for a, b in zip(there, back)])
    # the runs of stepless paths with five slots either side, for budgets below a path's steps (run_budget_cases)
    near = sorted(set(range(0, 9)) | set(range(at_tile - 5, at_tile + 9)) | set(range(at_two - 5, at_two + 7)) | set(range(P - 9, P)))
    s.add("around_the_runs", *listed(near))
    s.notes["near"] = near
    return s


def walked_steps(pools, pid: int, ws: int, we: int, m: int = 0):
    """(how many steps k_intervals walks for [ws, we) with M = m -- the steps from the first that ends at or past
    max(ws + 1, m) on, as long as they begin below we -- and how many of those have no length)"""
    r1 = ends_of(pools, pid)
    r0 = [0] + r1[:-1]
    if we <= ws:
        return 0, 0
    first = next((j for j, e in enumerate(r1) if e >= max(ws + 1, m)), len(r1))
    js = [j for j in range(first, len(r1)) if r0[j] < we]
    assert js == list(range(first, first + len(js)))
    return len(js), sum(1 for j in js if r1[j] == r0[j])


def cut_edges() -> Shape:
    """The lane / wave cut and k_long's rounds, aimed at: intervals that walk exactly 7, 8 and 9 steps (LANE_CUT - 1, LANE_CUT,
    LANE_CUT + 1), from a step seam and from inside a step, ending one base into their last step and at its end, with 0, 2 and 3
    of the walked steps of no length; paths of exactly 64 and 128 steps taken whole, from their second base and past their
    end, so that a wave's round ends on the path's last step."""
    rng = np.random.default_rng(22)
    lens = np.array([0, 3, 4, 2, 1, 5, 2], np.int64)
    segs = np.concatenate([rng.integers(0, 7, 500), [2], rng.integers(0, 7, 63), [5], rng.integers(0, 7, 127)])
    s = Shape("cut_edges", make_pools(lens, np.asarray(segs << 1, np.uint32), [(0, 500), (500, 564), (564, 692), (692, 692)]))
    r1 = ends_of(s.pools, 0)
    r0 = [0] + r1[:-1]
    n = len(r1)
    for k in (LANE_CUT - 1, LANE_CUT, LANE_CUT + 1):
        for z in (0, 2, 3):
            for inside in (0, 1):
                # steps a .. a + k - 1, a and the last of them with a length, z of them without
                a = next(a for a in range(1, n - k) if r1[a] - r0[a] > inside and r1[a + k - 1] > r0[a + k - 1]
                         and sum(1 for j in range(a, a + k) if r1[j] == r0[j]) == z)
                ws = r0[a] + inside
                ends = sorted({r0[a + k - 1] + 1, r1[a + k - 1]})
                for we in ends:
                    assert walked_steps(s.pools, 0, ws, we) == (k, z), (k, z, inside)
                # every interval its own group (a stepless path in between): M is 0, and the count is the one asserted
                s.add("walk%d_zeros%d_%s" % (k, z, "inside" if inside else "seam"), [0, 3] * len(ends),
                      [x for we in ends for x in (ws, 0)], [x for we in ends for x in (we, 1)])
    for pid, count in ((1, 64), (2, 128)):
        e = ends_of(s.pools, pid)
        L = e[-1]
        assert len(e) == count and e[0] >= 2
        for label, (ws, we) in (("whole", (0, L)), ("from1", (1, L)), ("past", (0, L + 5))):
            assert walked_steps(s.pools, pid, ws, we)[0] == count
            s.add("p%d_%s" % (pid, label), pid, [ws], [we])
        s.add("p%d_all" % pid, [pid, 3, pid, 3, pid], [0, 0, 1, 0, 0], [L, 1, L, 1, L + 5])
    return s


SHAPES = [basic, zeros, tiles, many_groups, long_positions, long_groups, many_paths, cut_edges]


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


def plan_slots(groups, lengths, budget):
    """The batches' slots (plan_interval_batches, restated as plan_batches restates it): a list of path lists."""
    out, steps = [[]], 0
    for k, p in enumerate(groups):
        if (k and groups[k - 1] == p) or p in out[-1]:
            continue
        if out[-1] and steps + lengths[p] > budget:
            out.append([])
            steps = 0
        out[-1].append(p)
        steps += lengths[p]
    return out


def run_budget_cases():
    """(label, list of many_paths, budget, batches) where a batch cut meets a run of stepless paths.  A path of no steps never
    makes the plan cut (it adds nothing to the batch's steps), so a cut touches a run in two ways only.  Budget 1, on the
    list around the runs: a path of two steps or more is over the budget alone, the stepless path behind it starts a batch of
    no steps, and the path of two steps or more behind the run cuts again: the run is a whole batch, cut at both its ends.
    Budget 1024 or 2048, on the whole list: the first batch fills exactly, takes the run in behind its last step -- it ends
    on a tile seam in stepless slots -- and the path that starts at that step begins the next batch."""
    s = shape("many_paths")
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in s.pools.paths]
    out = []
    for label, name, budget in (("runs-budget1", "around_the_runs", 1), ("budget1024", "slot_order", TILE), ("budget2048", "there_and_back", 2 * TILE)):
        ids = s.lists[name][0]
        groups = [int(ids[k]) for k in np.flatnonzero(np.concatenate([[True], np.diff(ids.astype(np.int64)) != 0]))]
        out.append((label, name, budget, len(plan_slots(groups, lengths, budget))))
    return out


def big_products():
    """(pools, depth, ids, starts, ends) of raw arrays no handle loads: segment lengths and depths up to 2^32 - 1, so that
    (double)(depth * len) rounds (the product has up to 64 bits), and intervals whose (double)(end - start) rounds."""
    top = (1 << 32) - 1
    lens = np.array([top, (1 << 31) + 1, 3, 0, top - 2, 123456789, 1, (1 << 32) - 5], np.int64)
    depth = np.array([top, top - 2, 7, 5, (1 << 31) + 3, 987654321, top, (1 << 30) + 1], np.uint64)
    segs = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 3, 3, 4, 1, 7, 6, 5, 2, 0, 4, 7], np.int64)
    pools = chop_shapes.make_pools(lens, np.asarray(segs << 1, np.uint32), [(0, 20), (3, 20)], seq=False)
    rows = [(0, 0, (1 << 64) - 1), (1, 0, (1 << 64) - 1), (0, 1, (1 << 63) + 1), (1, 1, (1 << 63) + 1)]
    for pid in (0, 1):
        r1 = ends_of(pools, pid)
        r0 = [0] + r1[:-1]
        L = r1[-1]
        assert L > 1 << 35
        rows += [(pid, 0, L), (pid, 1, L + (1 << 60) + 1), (pid, 0, (1 << 53) + 1)]
        for j in range(len(r1)):
            if r1[j] - r0[j] > 8:   # inside one step
                rows += [(pid, r0[j] + 5, r0[j] + 7), (pid, r0[j] + 1, r1[j] - 1), (pid, r0[j], r1[j])]
    assert any(int(depth[x]) * int(lens[x]) > 1 << 63 for x in range(len(lens)))
    ids, st, en = [], [], []
    for k, (pid, a, b) in enumerate(rows):  # every row alone in its group: a row on the other path in front of it
        ids += [1 - pid, pid]
        st += [3, a]
        en += [3, b]
    # and groups of several: M from a huge end, and from a small one
    ids += [0, 0, 0, 1, 1, 1]
    st += [5, 1, 0, 0, 2, 1]
    en += [1 << 33, (1 << 63) + 1, (1 << 64) - 1, 7, (1 << 64) - 1, (1 << 63) + 1]
    return pools, depth, np.array(ids, np.uint32), np.array(st, np.uint64), np.array(en, np.uint64)
