"""Graphs with long segments, shaped so that the 64-bit sums of path depth carry into their upper word at one chosen place
of the kernels each (pollen_amd/csrc/depth_accum.hip, depth_device.hip), for the tests only.

  fused route    pass 2 (k_accum<false, 12, true>) scans a window's seg_len and depth * seg_len into the prefix table LW
                 (block_scan<unsigned long long, kPer>: KPER segments a thread, 64 * KPER a wave), sum_groups takes a
                 difference of LW per run record (at most RUN_CAP segments), adds a lane's records up, reduces eight items
                 at a time over the wave (wave_totals8_u64) and stores one partial per (item, window); k_path_reduce adds
                 an item's windows up, 64 at a time (wave_total_u64), and adds the result to its path atomically
  gather route   k_path_sums: `split` blocks of SUM_THREADS threads per requested path, BATCH steps a thread in flight;
                 thread sums, a __shfl_down tree per wave, four waves through LDS, one atomicAdd per block

Each factory returns a Shape: the graph (steps, path_begin, path_end, seg_len, S) and its carry sites -- (kind, ...) tuples
that verify() proves from the reports of tests/path_depth_model.py: the value named at the site is >= 2^32 and, where the
kind says so, every addend below it is < 2^32.  Precondition of every shape: each path's totals are below 2^64.
"""
from __future__ import annotations

import os
import re
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import chop_shapes
import path_depth_model as pm
from oracle import flatgfa_oracle as fo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pollen_amd", "csrc")

# the kernels' geometry, mirrored (tests/test_path_depth_model.py checks each against the source text)
WB = 12  # window bits of the fused route
W = 1 << WB
WB_LARGE, WB_LARGE_FROM = 13, 1024 * 4096  # above this many segments
ACC_THREADS = 1024
KPER = W // ACC_THREADS  # 4 segments a thread of block_scan
WAVE_SEGS = 64 * KPER  # 256
RUN_CAP = 1024
SUM_THREADS, BATCH = 256, 8
MAX_SPLIT, JOBS_PER_CU = 64, 16
REDUCE_LANES = 64  # windows k_path_reduce adds per trip
SHORT_MAX, TINY_MAX = 2048, 128  # steps: at most so many and a path may go to a wave-per-path kernel, not to k_scan
SHORT_MAX_SEGS = 1 << 20  # ... on graphs of at most so many segments
M32 = (1 << 32) - 1


def source_constants() -> Dict[str, int]:
    """The same numbers as the source text has them."""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(pat, s):
        m = re.search(pat, s)
        assert m, pat
        return int(m.group(1))
    acc, dev, fast, kh = text("depth_accum.hip"), text("depth_device.hip"), text("depth_fast.hip"), text("depth_fast_kernels.hpp")
    ph = text("depth_fast.hpp")  # (the constants the plan decides by)
    assert re.search(r"k_accum<false, 12, true>", text("depth_fast.hip") + acc), "the fused build: depth only, 4096-segment windows, PSUM"
    assert re.search(r"constexpr int kPer = kW / kAccThreads;", acc)
    assert re.search(r"for \(uint32_t wdw = lane; wdw < n_win; wdw \+= 64u\)", acc)
    assert re.search(r"fp->wb != 12 \|\| fp->acc_parts > 1 \|\| fp->n_more", fast)
    m = re.search(r"uint32_t wb = g\.n_segs <= (\d+)u \* (\d+)u \? (\d+)u : (\d+)u;", fast)
    assert m
    return {
        "WB": int(m.group(3)), "WB_LARGE": int(m.group(4)), "WB_LARGE_FROM": int(m.group(1)) * int(m.group(2)),
        "ACC_THREADS": one(r"constexpr int kAccThreads = (\d+);", kh),
        "RUN_CAP": one(r"e1x = rel \+ \(\(rec >> WB\) & (\d+)u\) \+ 1u", acc) + 1,
        "RUN_CAP_SCAN": one(r"lenm1\[k\] = \(s\[k\]\.y - e\[k\]\.y - 1u\) & (\d+)u;", text("depth_scan.hip")) + 1,
        "SUM_THREADS": one(r"constexpr int kSumThreads = (\d+);", dev), "BATCH": one(r"constexpr int kBatch = (\d+);", dev),
        "MAX_SPLIT": one(r"split = std::max<uint32_t>\(1u, std::min<uint32_t>\((\d+)u, \(uint32_t\)\(pl->n_cus \* \d+\) / n_ids\)\);", dev),
        "JOBS_PER_CU": one(r"split = std::max<uint32_t>\(1u, std::min<uint32_t>\(\d+u, \(uint32_t\)\(pl->n_cus \* (\d+)\) / n_ids\)\);", dev),
        "SHORT_MAX": one(r"constexpr uint32_t kShortMax = (\d+);", ph), "TINY_MAX": one(r"constexpr uint32_t kTinyMax = (\d+);", ph),
        "SHORT_MAX_SEGS": 1 << one(r"constexpr uint32_t kShortMaxSegs = 1u << (\d+);", kh),
    }


class Shape(NamedTuple):
    name: str
    steps: np.ndarray  # uint32
    begin: np.ndarray  # uint32[P]
    end: np.ndarray
    seg_len: np.ndarray  # uint32[S]
    n_segs: int
    sites: Tuple[tuple, ...]
    env: Tuple[Tuple[str, str], ...] = ()  # what the fused configuration needs beyond the usual (piece size, ...)
    short_max0: bool = True  # every path an item of k_scan (FLATGFA_SHORT_MAX=0); False: the plan's own classes
    requests: Tuple[Tuple[str, tuple], ...] = ()  # gather shapes: (name, path ids in request order)

    @property
    def P(self) -> int:
        return len(self.begin)

    def graph(self):
        return self.steps, self.begin, self.end, self.seg_len, self.n_segs


def pools_of(s: Shape) -> fo.Pools:
    """The shape as the oracle's pools: segment s's sequence span is [0, seg_len[s]) of a pool that is not there (the depth
    oracle reads spans, never bases)."""
    return chop_shapes.make_pools(s.seg_len, s.steps, np.stack([s.begin, s.end], 1), seq=False)


class Builder:
    def __init__(self, n_segs: int, seed: int, lo: int = 1, hi: int = 9):
        self.S = n_segs
        self.rng = np.random.default_rng(seed)
        self.len = self.rng.integers(lo, hi + 1, n_segs).astype(np.uint64)
        self.paths: List[np.ndarray] = []

    def path(self, segs, rev=None) -> int:
        segs = np.asarray(segs, np.int64)
        assert len(segs) == 0 or (0 <= segs.min() and segs.max() < self.S)
        o = self.rng.integers(0, 2, len(segs)) if rev is None else np.full(len(segs), int(rev))
        self.paths.append(((segs << 1) | o).astype(np.uint32))
        return len(self.paths) - 1

    def shape(self, name, sites, **kw) -> Shape:
        n = np.array([len(p) for p in self.paths], np.int64)
        gap = 3  # bait steps (the graph's last segment) around every span: a kernel that reads past a span adds them
        steps, begin, end = [], [], []
        bait = np.full(gap, (self.S - 1) << 1, np.uint32)
        at = 0
        for p in self.paths:
            steps += [bait, p]
            at += gap
            begin.append(at)
            at += len(p)
            end.append(at)
        steps.append(bait)
        assert (self.len <= M32).all()
        return Shape(name, np.concatenate(steps).astype(np.uint32), np.array(begin, np.uint32), np.array(end, np.uint32),
                     self.len.astype(np.uint32), self.S, tuple(sites), **kw)


def crossing(lens: np.ndarray, lo: int, at: int, n: int) -> None:
    """Sets lens[lo : lo + n] so that their prefix sum first reaches 2^32 with segment lo + at (at >= 1): small lengths, a
    large one at the window's first segment and the rest of 2^32 at `at`."""
    lens[lo:lo + n] = 3
    lens[lo] = 1 << 31
    below = int(lens[lo:lo + at].sum())
    lens[lo + at] = (1 << 32) - below
    assert below < (1 << 32) <= below + int(lens[lo + at]) and lens[lo + at] <= M32


# ---- fused route ----
def prefix_len() -> Shape:
    """LW's length column passes 2^32: behind a window's first segment (of 2^32 - 1 bases), at its last, at a thread's first
    segment, at a wave's first, and at the last valid segment of the graph's last, partial window (nvalid 100)."""
    S = 6 * W + 100
    b = Builder(S, 1)
    b.len[W] = M32  # window 1: LW[1] = 2^32 - 1, LW[2] beyond
    crossing(b.len, 2 * W, W - 1, W)
    crossing(b.len, 3 * W, 5 * KPER, W)
    crossing(b.len, 4 * W, 3 * WAVE_SEGS, W)
    crossing(b.len, 6 * W, 99, 100)
    b.path(np.arange(S), rev=0)  # one path along everything: 1024-segment records
    b.path(np.arange(S - 1, -1, -1), rev=1)  # and back
    for w in range(7):  # short stretches inside every window, across each crossing
        lo, n = w * W, min(W, S - w * W)
        for a, c in ((0, 3), (n - 3, n), (5 * KPER - 2, 5 * KPER + 2), (3 * WAVE_SEGS - 2, 3 * WAVE_SEGS + 1), (n // 2, n // 2 + 40)):
            if 0 <= a < c <= n:
                b.path(np.arange(lo + a, lo + c), rev=0)
    sites = [("prefix", "len", 1, 1), ("prefix", "len", 2, W - 1), ("prefix", "len", 3, 5 * KPER), ("prefix", "len", 4, 3 * WAVE_SEGS),
             ("prefix", "len", 6, 99), ("nvalid", 6, 100)]
    return b.shape("prefix_len", sites)


def bit31() -> Shape:
    """Totals whose LOW word has bit 31 set, the high word 0, 1 or 2 -- and their neighbours below 2^31: the regression case of
    wave_total_u64's last step, which put the low word's sign over the high word (k_path_reduce)."""
    S = 3 * W
    b = Builder(S, 16)
    b.len[[10, 20, 30, 40, 41, 50, 51, 52]] = [(1 << 31) - 1, 1 << 31, M32, M32, (1 << 31) + 1, M32, M32, (1 << 31) + 2]
    sites = []
    b.path([10], rev=0)
    for segs in ([20], [30], [40, 41], [50, 51, 52], [10, 11, 12, 9]):
        sites.append(("bit31", "len", b.path(segs, rev=0)))
    b.len[W + 5] = 1 << 29
    for _ in range(4):
        p = b.path([W + 5], rev=1)  # depth 4: the weighted sum is 2^31, the length 2^29
    sites.append(("bit31", "w", p))
    return b.shape("bit31", sites)


def prefix_weighted() -> Shape:
    """Modest lengths (2^16), depth 17 to 48: LW's weighted column passes 2^32 in every window, its length column in none."""
    S = 3 * W + 5
    b = Builder(S, 2, 1 << 16, (1 << 16) + 99)
    for k in range(16):
        b.path(np.arange(S), rev=k & 1)
    for k in range(32):
        b.path(np.arange(W + 7 * k, 2 * W - 3 * k))
    b.path([5, 4097, 9000])
    return b.shape("prefix_weighted", [("prefix_w_only", w) for w in range(3)])


def runs() -> Shape:
    """One run record whose own sums pass 2^32 (a lane's share is at least its record): runs of 2, 1023 and 1024 segments and
    one that ends at its window's last segment in length; a run of ONE segment in the weighted sum (depth 3)."""
    S = 6 * W
    b = Builder(S, 3)
    sites = []
    for k, (first, n) in enumerate(((10, 2), (W + 100, 1023), (2 * W + 2048, 1024), (4 * W - 700, 700))):
        b.len[first:first + n] = (1 << 32) // n + 1 if n > 2 else M32
        sites.append(("run", "len", b.path(np.arange(first, first + n), rev=0), n))
    one = 4 * W + 17
    b.len[one] = M32 - 4
    for _ in range(3):
        sites.append(("run", "w", b.path([one], rev=0), 1))
    b.path([one + 2, one - 2, one + 4])
    return b.shape("runs", sites)


RECORD_COUNTS = (2, 3, 4, 8, 16, 32, 64, 65, 200)


def wave_totals() -> Shape:
    """Every lane's share below 2^32, the item's total in the window above: items of 2 .. 200 one-segment records (every
    other segment, so that no two join a run), each of 2^32 / R + 1 bases."""
    S = 12 * W
    b = Builder(S, 4)
    sites = []
    for k, R in enumerate(RECORD_COUNTS):
        lo = (k + 1) * W + 64
        segs = lo + 2 * np.arange(R)
        b.len[segs] = (1 << 32) // R + 1
        sites.append(("wave_total", "len", b.path(segs, rev=0), k + 1))
    return b.shape("wave_totals", sites)


def many_items(n_paths: int = 64 * 16 + 13 * 16 + 5) -> Shape:
    """More than 64 items a wave of one window's workgroup (16 waves): 1237 paths of two or three one-segment records in
    window 1, each record of 2^31 + 1 bases -- every item's total there passes 2^32, no lane's share does; items land at
    every position of sum_groups' groups of eight, and the last group of a stretch is not full."""
    S = 3 * W + 9
    b = Builder(S, 5)
    b.len[W:2 * W:2] = (1 << 31) + 1
    sites = []
    for p in range(n_paths):
        R = 2 + p % 2
        segs = W + 2 * ((p * 37 + 501 * np.arange(R)) % (W // 2))
        assert len(set(segs.tolist())) == R
        b.path(segs, rev=0)
        if p % 97 == 0:
            sites.append(("wave_total", "len", p, 1))
    return b.shape("many_items", sites)


def path_reduce() -> Shape:
    """Per-window partials below 2^32, the path's total above: a path over 70 windows (k_path_reduce's lanes take two windows
    each for the first six) with 2^26 bases in each; a second one with 2^31 per window, so that those lanes' own sums pass."""
    nw = 70
    S = nw * W + 7
    b = Builder(S, 6)
    a = np.arange(nw) * W + 33
    c = np.arange(nw) * W + 2000
    b.len[a] = 1 << 26
    b.len[c] = 1 << 31
    p0 = b.path(a, rev=0)
    p1 = b.path(c[::-1], rev=1)
    p2 = b.path(np.concatenate([a[:65], c[60:]]))
    return b.shape("path_reduce", [("path_reduce", "len", p0, nw), ("path_reduce", "len", p1, nw), ("path_reduce", "len", p2, nw)])


def split_paths() -> Shape:
    """Paths cut into pieces of 4096 steps (FLATGFA_PIECE_STEPS): every piece's sums below 2^32, their total above -- the
    pieces meet in k_path_reduce's atomicAdd."""
    S = 5 * W
    b = Builder(S, 7, 1 << 17, 1 << 18)
    p0 = b.path(np.arange(30_000) % S, rev=0)
    p1 = b.path(b.rng.integers(0, S, 26_000))
    b.path(np.arange(300))
    return b.shape("split_paths", [("split", "len", p0, 4096), ("split", "len", p1, 4096)], env=(("FLATGFA_PIECE_STEPS", "4096"),))


def reverse_nonmonotone() -> Shape:
    """Reverse-strand walks, random walks and walks that come back on themselves: short runs, many records, 2^24-2^25 bases a
    segment."""
    S = 4 * W + 77
    b = Builder(S, 8, 1 << 24, 1 << 25)
    sites = []
    sites.append(("total", "len", b.path(np.arange(S - 1, -1, -1), rev=1)))
    sites.append(("total", "len", b.path(b.rng.integers(0, S, 5000))))
    z = np.arange(3000)
    sites.append(("total", "len", b.path(W + np.where(z & 1, z + 3, z))))  # 0, 4, 2, 6, 4, 8, ...
    sites.append(("total", "len", b.path(np.concatenate([np.arange(500, 900), np.arange(900, 500, -1), np.arange(500, 900)]))))
    sites.append(("total", "len", b.path(np.repeat(np.arange(2 * W - 50, 2 * W + 50), 3))))
    return b.shape("reverse_nonmonotone", sites)


def beyond_2_53(n_steps: int = (1 << 21) + 4099) -> Shape:
    """length beyond 2^53 (2^21 + 4099 steps over segments near 2^32 - 1) and weighted sums of 2^64 - 1, - 1001 and - 3001
    (one segment of 2^32 - 1 bases 65536 times: 2^64 - 2^32, and one of 2^32 - 1 - k once): the division rounds both."""
    S = 3 * W
    b = Builder(S, 9)
    b.len[:W] = M32 - (np.arange(W) % 7).astype(np.uint64)
    p0 = b.path(np.arange(n_steps) % W, rev=0)
    sites = [("beyond53", "len", p0)]
    for j, k in enumerate((0, 1000, 3000)):
        a, c = W + 10 + 4 * j, W + 12 + 4 * j
        b.len[a], b.len[c] = M32, M32 - k
        p = b.path(np.concatenate([np.full(1 << 16, a), [c]]), rev=0)
        sites.append(("near64", p, (1 << 64) - 1 - k))
    return b.shape("beyond_2_53", sites)


def zeros() -> Shape:
    """Segments of no bases among long ones, paths over empty segments only (0 / 0: NaN) and paths of no steps."""
    S = 2 * W + 300
    b = Builder(S, 10, 0, 2)
    b.len[::3] = 0
    b.len[1000:1100] = 0
    b.len[7] = M32
    b.len[2000] = M32
    sites = [("nan", b.path(np.arange(1000, 1100), rev=0)), ("nan", b.path([])), ("nan", b.path([0, 3, 6, 0])), ("nan", b.path([]))]
    sites.append(("total", "len", b.path([7, 0, 2000, 3])))
    b.path(np.arange(S))
    sites.append(("nan", b.path([])))
    return b.shape("zeros", sites)


def large_windows() -> Shape:
    """More than 4 Mi segments: 8192-segment windows, a plan the fused route is not for.  Long runs through window 1 and the
    last full one (512), whose prefix sums pass 2^32 (proved with the shape's own window bits)."""
    S = WB_LARGE_FROM + 2 * W + 5
    b = Builder(S, 11, 1, 2)
    b.len[8192:8192 + 3000] = 1 << 22
    b.len[S - 2000:] = 1 << 23
    sites = [("total", "len", b.path(np.arange(8000, 12000), rev=0)), ("total", "len", b.path(np.arange(S - 1, S - 1800, -1), rev=1)),
             ("total", "len", b.path(b.rng.integers(S - 2000, S, 3000)))]
    b.path(b.rng.integers(0, S, 2000))
    sites += [("prefix_any", "len", 1), ("prefix_any", "len", WB_LARGE_FROM >> WB_LARGE)]
    return b.shape("large_windows", sites)


def host_long() -> Shape:
    """What a .flatgfa image can hold cheaply: 9000 segments of 2^20 .. 2^22 bases whose sequence spans all begin at offset 0 of
    one 4 MiB pool.  A walk along all of them (2^32 and more in every window's prefix), one back, random and short ones."""
    S = 9000
    b = Builder(S, 15, 1 << 20, 1 << 22)
    sites = [("total", "len", b.path(np.arange(S), rev=0)), ("total", "len", b.path(np.arange(S - 1, -1, -1), rev=1)),
             ("total", "len", b.path(b.rng.integers(0, S, 6000))), ("total", "len", b.path(np.arange(100, 2300), rev=0))]
    b.path([17, 18, 19])
    b.path([])
    sites.append(("prefix_any", "len", 0))
    return b.shape("host_long", sites, short_max0=False)


GATHER_STEPS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 64 * 2048 - 1, 64 * 2048 + 1)


def gather_lengths(n_cus: int = 256) -> Shape:
    """Paths of 0 .. 64 * 2048 + 1 steps over segments of 2^30-2^32 bases: the eight-deep loop of k_path_sums and its tail at
    every trip count, slices of no steps; requested alone (split 64), 16 CUs and 16 CUs + 1 times (split 1), several times
    that, with repeats, in descending order."""
    S = 5000
    b = Builder(S, 12, 1 << 30, M32)
    for n in GATHER_STEPS:
        b.path(b.rng.integers(0, S, n))
    P = len(GATHER_STEPS)
    full = JOBS_PER_CU * n_cus
    reqs = (("all", tuple(range(P))), ("one", (P - 1,)), ("descending", tuple(range(P - 1, -1, -1))), ("repeats", (3, 3, 12, 0, 3, 12, 1)),
            ("split1", tuple(i % P for i in range(full))), ("split1_plus", tuple((7 * i) % P for i in range(full + 1))),
            ("several", tuple((5 * i + 2) % P for i in range(3 * full + 5))))
    sites = [("gather_trips", p, MAX_SPLIT) for p in range(P)] + [("gather_trips", p, 1) for p in range(P)]
    return b.shape("gather_lengths", sites, requests=reqs, short_max0=False)


def gather_levels(n_cus: int = 256) -> Shape:
    """A thread's own sum, a wave's, a block's and the atomicAdd's target pass 2^32 in turn, each with the level below under
    it: uniform segments of 2^32 - 1, 2^24, 2^22 and 2^16 bases, paths of 4096, 2048, 2048 and 64 * 2048 steps; the first
    three are requested 16 CUs times (split 1: 8 or 16 addends a thread), the last alone (split 64)."""
    S = 4 * 1024
    b = Builder(S, 13)
    for k, L in enumerate((M32, 1 << 24, 1 << 22, 1 << 16)):
        b.len[k * 1024:(k + 1) * 1024] = L
    full = JOBS_PER_CU * n_cus
    p = [b.path(b.rng.integers(0, 1024, 4096)), b.path(1024 + b.rng.integers(0, 1024, 2048)), b.path(2048 + b.rng.integers(0, 1024, 2048)),
         b.path(3072 + b.rng.integers(0, 1024, 64 * 2048))]
    sites = [("gather_level", "thread", p[0], 1), ("gather_level", "wave", p[1], 1), ("gather_level", "block", p[2], 1),
             ("gather_level", "atomic", p[3], MAX_SPLIT)]
    reqs = tuple(("split1_p%d" % q, (q,) * full) for q in p[:3]) + (("split64", (p[3],)),)
    return b.shape("gather_levels", sites, requests=reqs, short_max0=False)


def mixed() -> Shape:
    """Long, medium, short and tiny paths in one graph of 2^16 segments: one path_depth_all call credits the long ones from
    k_path_reduce and the others from k_path_sums (the plan's other_ids); every total passes 2^32."""
    S = 1 << 16
    b = Builder(S, 14, 1 << 27, 1 << 29)
    sites = []
    for n in (40_000, 25_000, 9_000):  # k_scan's
        start = int(b.rng.integers(0, S))
        sites.append(("total", "len", b.path((start + np.arange(n)) % S, rev=0)))
    for n in (2048, 1500, 700, 300, 129):  # a wave each: short or medium
        sites.append(("total", "len", b.path(b.rng.integers(0, S, n))))
    for n in (128, 64, 33):
        sites.append(("total", "len", b.path(int(b.rng.integers(0, S - 200)) + np.arange(n), rev=0)))
    b.path([5])
    b.path([])
    return b.shape("mixed", sites, short_max0=False)


FUSED = (bit31, prefix_len, prefix_weighted, runs, wave_totals, many_items, path_reduce, split_paths, reverse_nonmonotone, beyond_2_53, zeros)


def catalog(n_cus: int = 256) -> List[Tuple[str, Callable[[], Shape]]]:
    return [(f.__name__, f) for f in FUSED] + [("mixed", mixed), ("host_long", host_long), ("large_windows", large_windows),
                                               ("gather_lengths", lambda: gather_lengths(n_cus)), ("gather_levels", lambda: gather_levels(n_cus))]


EXACT_MAX_STEPS = 400_000  # shapes up to this size are run through the exact model (and its run report)


# ---- the proof of a shape's sites, from the model's reports ----
def verify(s: Shape, n_cus: int = 256) -> int:
    """Checks every declared site; returns how many it checked."""
    T = pm.TWO32
    small = len(s.steps) <= EXACT_MAX_STEPS
    ans = pm.exact(*s.graph()) if small else pm.twin(*s.graph())
    length, weighted = [int(x) for x in ans.length], [int(x) for x in ans.weighted]
    assert all(x < pm.TWO64 for x in length + weighted)  # the precondition
    d = ans.depth
    col = {"len": 0, "w": 1}
    rs: Optional[list] = None
    piece = int(dict(s.env).get("FLATGFA_PIECE_STEPS", 0))
    wb = pm.window_bits(s.n_segs)  # the shape's own windows: 8192 segments above 4 Mi

    def get_runs():
        nonlocal rs
        if rs is None:
            assert small, s.name
            rs = pm.runs(s.steps, s.begin, s.end, s.seg_len, d, wb, RUN_CAP, piece)
        return rs
    for site in s.sites:
        kind = site[0]
        if kind == "prefix":
            _, c, win, at = site
            LW = pm.window_prefix(s.seg_len, d, s.n_segs, wb, win)[col[c]]
            assert LW[at] < T <= LW[at + 1], (s.name, site, LW[at], LW[at + 1])
        elif kind == "nvalid":
            assert s.n_segs - (site[1] << wb) == site[2] and ((s.n_segs - 1) >> wb) == site[1]
        elif kind == "prefix_w_only":
            L, Wt = pm.window_prefix(s.seg_len, d, s.n_segs, wb, site[1])
            assert L[-1] < T <= Wt[-1], (s.name, site, L[-1], Wt[-1])
        elif kind == "run":
            _, c, p, n = site
            mine = [r for r in get_runs() if r.path == p]
            assert len(mine) == 1 and mine[0].n == n and mine[0][5 + col[c]] >= T, (s.name, site, mine[:3])
            if c == "w":
                assert mine[0].length < T
            if n > 1:  # (every addend below: a segment's own length, and its depth * length where the site is the weighted sum)
                assert all(int(s.seg_len[x]) * (int(d[x]) if c == "w" else 1) < T for x in range(mine[0].first, mine[0].first + n))
        elif kind == "wave_total":
            _, c, p, win = site
            part = pm.item_partials(get_runs())[(p, 0, win)][col[c]]
            shares = [x[col[c]] for x in pm.lane_shares(get_runs(), p, 0, win)]
            assert max(shares) < T <= part == sum(shares), (s.name, site, max(shares), part)
        elif kind == "path_reduce":
            _, c, p, nw = site
            parts = [v[col[c]] for (q, _, _), v in pm.item_partials(get_runs()).items() if q == p]
            assert len(parts) == nw > REDUCE_LANES and max(parts) < T <= sum(parts) == (length, weighted)[col[c]][p]
        elif kind == "split":
            _, c, p, steps = site
            assert steps == piece
            by_piece: Dict[int, int] = {}
            for (q, k, _), v in pm.item_partials(get_runs()).items():
                if q == p:
                    by_piece[k] = by_piece.get(k, 0) + v[col[c]]
            assert len(by_piece) == -(-int(s.end[p] - s.begin[p]) // piece) >= 3 and max(by_piece.values()) < T <= sum(by_piece.values())
        elif kind == "prefix_any":
            assert pm.window_prefix(s.seg_len, d, s.n_segs, wb, site[2])[col[site[1]]][-1] >= T
        elif kind == "bit31":
            assert (length, weighted)[col[site[1]]][site[2]] >> 31 & 1
        elif kind == "total":
            assert (length, weighted)[col[site[1]]][site[2]] >= T
        elif kind == "beyond53":
            v = (length, weighted)[col[site[1]]][site[2]]
            assert v > 1 << 53 and float(v) != v  # (the conversion really rounds)
        elif kind == "near64":
            assert weighted[site[1]] == site[2] and (1 << 64) - weighted[site[1]] <= 4 * 2048  # (an ulp below 2^64 is 2048)
        elif kind == "nan":
            assert length[site[1]] == 0 and weighted[site[1]] == 0 and np.isnan(ans.mean[site[1]])
        elif kind == "gather_trips":
            _, p, split = site
            n = int(s.end[p] - s.begin[p])
            g = [pm.gather_slice(s.steps, int(s.begin[p]), int(s.end[p]), s.seg_len, d, split, k, SUM_THREADS, BATCH) for k in {0, split - 1}]
            if split == 1:  # the trip counts the path's length was chosen for
                first = (BATCH - 1) * SUM_THREADS  # thread 0 makes a batch trip while its eighth step lies inside the slice
                nb = 0 if n <= first else -(-(n - first) // (SUM_THREADS * BATCH))
                assert g[0].n_batches == nb and g[0].n_tail == max(0, -(-(n - nb * SUM_THREADS * BATCH) // SUM_THREADS))
                assert g[0].block == (length[p], weighted[p])
            elif n < split:
                assert any(x.block == (0, 0) for x in g) or n == 0
        elif kind == "gather_level":
            _, level, p, split = site
            g = [pm.gather_slice(s.steps, int(s.begin[p]), int(s.end[p]), s.seg_len, d, split, k, SUM_THREADS, BATCH) for k in range(split)]
            th = max(a for x in g for a, _ in x.threads)
            wv = max(a for x in g for a, _ in x.waves)
            bl = max(x.block[0] for x in g)
            assert sum(x.block[0] for x in g) == length[p]
            addend = int(s.seg_len[s.steps[int(s.begin[p])] >> 1])
            chain = {"thread": (addend, th), "wave": (th, wv), "block": (wv, bl), "atomic": (bl, length[p])}[level]
            assert chain[0] < T <= chain[1], (s.name, site, chain)
            if split == 1:
                assert split == pm.split_of(JOBS_PER_CU * n_cus, n_cus)
        else:
            raise AssertionError(site)
    return len(s.sites)
