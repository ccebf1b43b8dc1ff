"""Graphs shaped around the grid strides, coarse blocks, LDS windows, query batches and limits of the path-overlap kernels
(pollen_amd/csrc/overlap_device.hip), for the tests only.

  k_coarse_bits   one workgroup per path, at most 16 per CU, grid-stride over the paths
  k_handle_bits   one workgroup per (query, orientation, window of WIN_WORDS words), at most 16 per CU, grid-stride
  k_pair_touch    one wave per (query, path), at most 64 workgroups of 4 waves per CU, grid-stride; its coarse test ANDs
                  the paths' bitmaps (one bit per BLOCK handles) 64 words a round
  the host        exact bitsets of every path when P * per_query <= 1 GB (all-paths mode, 2a), else of the queries only,
                  DENSE / per_query queries a batch (queries-only mode, 2b); more than MAX_SEGS segments: refused

Each factory returns a Shape: the steps, the spans, n_segs, the query ids and, for the planted shapes, the answer in closed
form -- the pairs the builder put a common handle into; every other handle of a planted shape is used by one path only.
Spans are laid out with at least four steps of a bait handle before and after each one and begin at every offset mod 4, so
a kernel that reads past a span finds the bait path (a query) there.  Shapes without a closed form (want None) are random
and checked against tests/overlap_model.py.  Sizes that depend on the device take its CU count.
"""
from __future__ import annotations

import os
import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pollen_amd", "csrc", "overlap_device.hip")


def _const(name: str) -> int:
    with open(HIP) as f:
        m = re.search(r"constexpr\s+u?int(?:32_t)?\s+%s\s*=\s*(\d+)" % name, f.read())
    assert m, name
    return int(m.group(1))


WIN_WORDS = _const("kBitsWinWords")  # 36864 words of LDS: one k_handle_bits pass
WIN_SEGS = 32 * WIN_WORDS  # 1,179,648 segments
BLOCK = 1 << _const("kBlockBits")  # 2048 handles a coarse bit
COARSE_MAX_WORDS = _const("kCoarseMaxWords")  # 8192
PAIR_THREADS = _const("kPairThreads")  # 256: 4 waves of 64
MAX_SEGS = COARSE_MAX_WORDS * 32 * BLOCK // 2  # 2^28
DENSE = 1 << 30  # the exact-bitset budget of one call (dense_max and the batch size)
# the launches' workgroups per CU (overlap_device.hip: n_cus * 16u, n_cus * 16u, n_cus * 64u)
COARSE_WG_PER_CU, BITS_WG_PER_CU, PAIR_WG_PER_CU = 16, 16, 64
BALLOT = 64  # coarse words a round of k_pair_touch's ballot loop
ERR_BOUNDS, ERR_TOO_LARGE = -2, -6
REFUSED = (MAX_SEGS + 1, 1 << 31, (1 << 32) - 32, (1 << 32) - 31, (1 << 32) - 1)


# ---- the host's arithmetic, in Python ints ----
def words(S: int) -> int:
    return ((S + 31) // 32 + 3) & ~3


def cwords(S: int) -> int:
    return ((2 * S + BLOCK - 1) // BLOCK + 31) // 32


def n_win(S: int) -> int:
    return (words(S) + WIN_WORDS - 1) // WIN_WORDS


def per_query(S: int) -> int:
    return 8 * words(S)


def all_paths(S: int, P: int, dense_max: int = DENSE) -> bool:
    return P * per_query(S) <= dense_max


def batches(S: int, P: int, n_q: int, dense_max: int = DENSE) -> List[Tuple[int, int]]:
    """The (q0, nq) of each k_pair_touch launch of one call."""
    if all_paths(S, P, dense_max):
        return [(0, n_q)]
    b = max(1, min(n_q, DENSE // per_query(S)))
    return [(q0, min(b, n_q - q0)) for q0 in range(0, n_q, b)]


class Shape(NamedTuple):
    name: str
    steps: np.ndarray  # uint32
    begin: np.ndarray  # uint32[P]
    end: np.ndarray
    n_segs: int
    queries: np.ndarray  # uint32[n_q]
    want: Optional[np.ndarray] = None  # uint8[n_q, P] in closed form; None: the model's
    dense_max: int = DENSE  # (a shape may ask for queries-only mode through the hook)

    @property
    def P(self) -> int:
        return len(self.begin)


class Planted:
    """A graph built path by path.  plant(h, paths) puts handle h into each of those paths and records every pair of them
    as touching; fill(p, n) gives path p n handles nobody else has; layout() lays the paths out between bait steps."""

    def __init__(self, n_segs: int, seed: int, bait_seg: int = 5):
        self.S = n_segs
        self.rng = np.random.default_rng(seed)
        self.paths: List[List[int]] = []
        self.pairs = set()
        self.used = set()
        self.bait = 2 * bait_seg
        self.used.update((self.bait, self.bait + 1))
        self.bait_path = self.new_path()
        self.paths[self.bait_path].append(self.bait)
        self.extra: List[Tuple[int, int]] = []  # spans given by hand, in steps of the raw block (see raw())
        self.raw_block: List[int] = []

    def new_path(self, n: int = 1) -> int:
        self.paths.extend([] for _ in range(n))
        return len(self.paths) - n

    def plant(self, h: int, paths: Sequence[int]) -> None:
        assert 0 <= h >> 1 < self.S and h not in self.used, h
        self._plant(h, paths)

    def plant_new(self, paths: Sequence[int], lo_seg: int = 0, hi_seg: Optional[int] = None) -> int:
        """plant() of a handle of a segment in [lo_seg, hi_seg) that no path has yet."""
        h = self.unique(1, lo_seg, hi_seg)[0]
        self._plant(h, paths)
        return h

    def _plant(self, h: int, paths: Sequence[int]) -> None:
        self.used.add(h)
        for p in paths:
            self.paths[p].append(h)
        ps = sorted(set(paths))
        self.pairs.update((a, b) for a in ps for b in ps if a != b)

    def unique(self, n: int, lo_seg: int = 0, hi_seg: Optional[int] = None) -> List[int]:
        """n handles of segments in [lo_seg, hi_seg) that no path has yet (marked used)."""
        hi_seg = self.S if hi_seg is None else hi_seg
        out = []
        while len(out) < n:
            h = int(self.rng.integers(2 * lo_seg, 2 * hi_seg))
            if h not in self.used:
                self.used.add(h)
                out.append(h)
        return out

    def fill(self, p: int, n: int, lo_seg: int = 0, hi_seg: Optional[int] = None) -> None:
        self.paths[p].extend(self.unique(n, lo_seg, hi_seg))

    def raw(self, handles: Sequence[int], spans: Sequence[Tuple[int, int]], pairs: Sequence[Tuple[int, int]]) -> List[int]:
        """Paths whose spans are given by hand over one block of steps (overlapping, nested, identical, empty): `spans` index
        `handles`, `pairs` the touching pairs among them (by position in `spans`).  Returns the new path ids."""
        for h in handles:
            assert h not in self.used
        self.used.update(handles)
        base = len(self.raw_block)
        self.raw_block.extend(handles)
        ids = []
        for b, e in spans:
            ids.append(self.new_path())
            self.extra.append((ids[-1], base + b, base + e))
        for a, b in pairs:
            self.pairs.update(((ids[a], ids[b]), (ids[b], ids[a])))
        return ids

    def layout(self, shuffle: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        steps: List[int] = []
        P = len(self.paths)
        begin, end = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
        by_hand = {p for p, _, _ in self.extra}
        for p in range(P):
            if p in by_hand:
                continue
            gap = 4 + (p - len(steps) - 4) % 4  # (span p begins at offset p mod 4 of a 16-byte line)
            steps.extend([self.bait] * gap)
            hs = list(self.paths[p])
            if shuffle:
                self.rng.shuffle(hs)
            begin[p] = len(steps)
            steps.extend(hs)
            end[p] = len(steps)
        if self.extra:
            steps.extend([self.bait] * 4)
            base = len(steps)
            steps.extend(self.raw_block)
            for p, b, e in self.extra:
                begin[p], end[p] = base + b, base + e
        steps.extend([self.bait] * 4)
        return np.array(steps, np.uint32), begin, end

    def answer(self, queries) -> np.ndarray:
        P = len(self.paths)
        m = np.zeros((P, P), np.uint8)
        if self.pairs:
            a, b = np.array(sorted(self.pairs)).T
            m[a, b] = 1
        return m[np.asarray(queries, np.int64)]

    def shape(self, name: str, queries=None, dense_max: int = DENSE, shuffle: bool = True) -> Shape:
        steps, b, e = self.layout(shuffle)
        q = np.arange(len(self.paths), dtype=np.uint32) if queries is None else np.asarray(queries, np.uint32)
        return Shape(name, steps, b, e, self.S, q, self.answer(q), dense_max)


# ---- random graphs past the grid strides (answer: the model) ----
def hot_graph(name, S, P, seed, max_len=40, n_hot=2000, queries=None) -> Shape:
    """P paths of 1..max_len steps; about half the steps are one of n_hot handles spread over the whole handle range (so
    pairs touch), the rest uniform over it."""
    rng = np.random.default_rng(seed)
    hot = rng.choice(2 * S, n_hot, replace=False).astype(np.uint32)
    n = rng.integers(1, max_len + 1, P)
    N = int(n.sum())
    steps = np.where(rng.random(N) < 0.5, hot[rng.integers(0, n_hot, N)], rng.integers(0, 2 * S, N)).astype(np.uint32)
    end = np.cumsum(n).astype(np.uint32)
    begin = (end - n).astype(np.uint32)
    q = np.arange(P, dtype=np.uint32)[::-1].copy() if queries is None else np.asarray(queries, np.uint32)
    return Shape(name, steps, begin, end, S, q)


def grid_batches(n_cus: int = 256) -> Shape:
    """S = 3 * 2^20 + 5 (three windows), P = max(5000, 16 CUs + 904) paths: past k_coarse_bits' stride; queries-only (P * 786 KB >
    1 GB) in batches of 1365 whose jobs (x 6) and pairs (x P) are past the strides of the other two kernels."""
    return hot_graph("grid_batches", 3 * (1 << 20) + 5, max(5000, COARSE_WG_PER_CU * n_cus + 904), seed=11)


def grid_dense(n_cus: int = 256) -> Shape:
    """S = 2^16 + 3, P as grid_batches': all-paths mode (82 MB of bitsets) with P * 2 jobs past k_handle_bits' stride;
    700 queries with repeats."""
    S, P = (1 << 16) + 3, max(5000, COARSE_WG_PER_CU * n_cus + 904)
    rng = np.random.default_rng(12)
    q = np.concatenate([rng.choice(P, 690, replace=False), [0, P - 1, P - 1, 7, 7, 7, 0, 1, 2, 3]]).astype(np.uint32)
    return hot_graph("grid_dense", S, P, seed=12, n_hot=800, queries=q)


# ---- planted shapes ----
def edges(S: int = 3 * (1 << 21) + 4099, seed: int = 21) -> Shape:
    """Coarse-block edges (handles 2047 / 2048), the last partial block, coarse words 64 and on (segments >= 2^21, paths
    with no block in common below), window edges k * WIN_SEGS - 1 / k * WIN_SEGS, a query only in a later window, and
    orientation.  At the default S: cwords 193, words 196740 (not a multiple of 32), 6 windows."""
    b = Planted(S, seed)
    two = lambda: [b.new_path(), b.new_path()]  # noqa: E731
    fills = []  # (after every planted handle: a filler never takes one)
    low_fill = (10_000, (1 << 21) - 10_000)  # fillers stay below 2^21
    top = 2 * S - 1
    for h in (BLOCK - 1, BLOCK, top, top - 1, 0, 1):  # block edges, last block, first block
        pq = two()
        b.plant(h, pq)
        fills.append((pq[0], 3) + low_fill)
    for h in (BLOCK - 2, BLOCK + 1, top - 2, top - 3):  # a block in common with the pairs above, no handle
        b.plant(h, [b.new_path()])
    # one segment in opposite orientations: never a touch; a reverse handle shared: a touch
    s = 3 * BLOCK + 17
    pq = two()
    b.plant(2 * s, [pq[0]])
    b.plant(2 * s + 1, [pq[1]])
    b.plant(2 * s + 3, pq)  # (s + 1, reverse)
    # the second and later rounds of the coarse ballot: nothing in common below segment 2^21
    cw = cwords(S)
    for w in sorted({BALLOT, BALLOT + 1, 2 * BALLOT, cw - 1}):
        if w >= cw:
            continue
        first = w * 32 * BLOCK  # the first handle of coarse word w
        for h in (first, first + 32 * BLOCK - 1 if w < cw - 1 else top - 4):
            pq = two()
            b.plant(h, pq)
            fills.append((pq[1], 2, (first >> 1) + 1, min(S, (first >> 1) + 16 * BLOCK)))
    h = BALLOT * 32 * BLOCK - 1  # the last handle of round one
    if (h >> 1) < S:
        pq = two()
        b.plant(h, pq)
    # windows: the last segment of window k - 1 and the first of window k, both orientations
    nw = n_win(S)
    for k in sorted({1, 2, nw - 1}):
        for s in (k * WIN_SEGS - 1, k * WIN_SEGS):
            if s >= S:
                continue
            for o in (0, 1):
                pq = two()
                b.plant(2 * s + o, pq)
    if nw >= 4:  # a query whose handles all lie in window 3
        q = b.new_path(3)
        c, d = q + 1, q + 2
        s = 3 * WIN_SEGS + 999
        b.plant(2 * s, [q, c])
        b.plant(2 * s + 7, [q, d])
        b.plant(2 * s + 9, [q])
    # one path on many of the above: touches each of them, each through a handle of its own below 2^21
    hub = b.new_path()
    for p in range(1, hub, 5):
        b.plant_new([hub, p], 2 * BLOCK, low_fill[0])
    for f in fills:
        b.fill(*f)
    q = np.arange(len(b.paths), dtype=np.uint32)
    q = np.concatenate([q, [0, 3, 3, len(b.paths) - 1]]).astype(np.uint32)
    return b.shape("edges", q)


def orientation(S: int = 4099, seed: int = 22) -> Shape:
    """Pairs that share only reverse handles (touch), only forward ones (touch), and pairs that share segments only in
    opposite orientations (no touch), many to a coarse block."""
    b = Planted(S, seed)
    for i in range(40):
        s = 100 + 37 * i
        pq = [b.new_path(), b.new_path()]
        kind = i % 3
        if kind == 0:
            b.plant(2 * s + 1, pq)
        elif kind == 1:
            b.plant(2 * s, pq)
        else:
            b.plant(2 * s, [pq[0]])
            b.plant(2 * s + 1, [pq[1]])
        b.plant(2 * (s + 1) + (i & 1), [pq[0]])
        b.plant(2 * (s + 1) + 1 - (i & 1), [pq[1]])
    return b.shape("orientation")


def step_layout(S: int = 3001, seed: int = 23) -> Shape:
    """Paths of 0..7 steps at every begin offset mod 4 beside four query paths they share a handle with (or not), between
    bait steps; overlapping, nested and identical spans; empty paths; a path that repeats handles nobody else has."""
    b = Planted(S, seed)
    qs = [b.new_path(4) + i for i in range(4)]
    for i in range(8):  # the queries also touch each other a little
        b.plant_new([qs[i % 4], qs[(i * 3 + 1) % 4]], 1000, 1100)
    for L in range(8):
        for share in (False, True):
            for off in range(4):  # (consecutive paths: every begin offset mod 4)
                p = b.new_path()
                n_fill = L - (1 if share and L else 0)
                b.fill(p, n_fill, 1100, S)
                if share and L:
                    b.plant_new([p, qs[(L + off) % 4]], 200, 1000)
    rep = b.new_path()
    r = b.unique(1, 1100, S)[0]
    b.paths[rep].extend([r] * 9)  # repeats, shared with no other path
    e0 = b.new_path()  # an empty path between the others
    raw = [b.unique(1, 1100, S)[0] for _ in range(8)]
    b.used.difference_update(raw)  # (raw() takes them)
    # spans over raw[0..8): O1 = [0,4), O2 = [2,6), O3 = [1,3) (in O1), O4 = [0,4) (= O1), O5 = [4,6), O6 = [6,8) + empty ones
    spans = [(0, 4), (2, 6), (1, 3), (0, 4), (4, 6), (6, 8), (3, 3), (8, 8)]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (1, 4)]
    ids = b.raw(raw, spans, pairs)
    b.paths[qs[0]].append(raw[7])  # (O6 holds raw[7])
    b.pairs.update(((ids[5], qs[0]), (qs[0], ids[5])))
    q = np.array(list(range(len(b.paths))) + [e0, ids[6], qs[2], qs[2]], np.uint32)
    assert len(b.paths[e0]) == 0
    return b.shape("step_layout", q)


def batch_edges(n_q: int = 1200, P: int = 1200, S: int = 8 * (1 << 20), seed: int = 24) -> Shape:
    """S = 2^23: words 2^18, 2 MiB a query, batches of 512 -- 512, 512, 176 for 1200 queries, reached without the hook.
    Path queries[k] touches path queries[k + 1] across the batch edges; repeated query ids sit in different batches."""
    b = Planted(S, seed)
    b.new_path(P - 1)
    rng = b.rng
    q = rng.permutation(np.arange(1, P))[: n_q - 1].tolist()
    q.insert(300, 0)  # (the bait path is a query)
    bsz = DENSE // per_query(S)
    for pos, src in ((bsz + 10, 100), (2 * bsz + 5, 700), (2 * bsz + 6, 100), (bsz - 1, 3)):
        if pos < n_q:
            q[pos] = q[src]
    for k in (bsz - 2, bsz - 1, bsz, 2 * bsz - 1, 2 * bsz):
        if k + 1 < n_q and q[k] != q[k + 1]:
            b.plant_new([q[k], q[k + 1]])
    for _ in range(300):  # and pairs anywhere, in every window
        b.plant_new(rng.choice(np.arange(1, P), int(rng.integers(2, 4)), replace=False).tolist())
    for p in range(1, P):
        b.fill(p, int(rng.integers(0, 12)))
    return b.shape("batch_edges", q)


def limit(P: int = 24, S: int = MAX_SEGS, seed: int = 25) -> Shape:
    """S = 2^28 exactly: cwords 8192, words 2^23, 64 MiB a query, batches of 16, 228 windows.  Handles on the top handle,
    the first, block edges and window edges (k = 1, 2, 100, last); more than 16 paths: queries-only."""
    b = Planted(S, seed)
    b.new_path(P - 1)
    nw = n_win(S)
    hs = [2 * S - 1, 2 * S - 2, 0, 1, BLOCK - 1, BLOCK, 2 * S - BLOCK, 2 * S - BLOCK - 1]
    for k in (1, 2, 100, nw - 1):
        hs += [2 * (k * WIN_SEGS) - 1, 2 * (k * WIN_SEGS), 2 * (k * WIN_SEGS) + 1]
    for i, h in enumerate(hs):
        a = 1 + i % (P - 1)
        c = 1 + (7 * i + 3) % (P - 1)
        b.plant(h, [a] if a == c else [a, c])
    for p in range(1, P):
        b.fill(p, 3)
    q = list(range(P)) + [P - 1, 5]
    return b.shape("limit" if P > 16 else "limit_dense", q)


def limit_dense() -> Shape:
    """The same with 16 paths: all of them fit 1 GB of exact bitsets (all-paths mode over 8192 coarse words)."""
    return limit(P=16, seed=26)


def refused(S: int) -> Shape:
    """Two paths of one step each over S segments: a graph the overlap call refuses before it launches anything."""
    steps = np.array([0, 2], np.uint32)
    return Shape("refused_%d" % S, steps, np.array([0, 1], np.uint32), np.array([1, 2], np.uint32), S, np.array([0, 1], np.uint32))


def catalog(n_cus: int = 256):
    """(name, factory) of every shape the device runs, cheapest first."""
    return [
        ("orientation", orientation),
        ("step_layout", step_layout),
        ("grid_dense", lambda: grid_dense(n_cus)),
        ("edges", edges),
        ("grid_batches", lambda: grid_batches(n_cus)),
        ("batch_edges", batch_edges),
        ("limit_dense", limit_dense),
        ("limit", limit),
    ]
