"""Graphs shaped around the tiles and the 32-bit limits of the GPU chop (pollen_amd/csrc/chop_device.hip), for the tests only.

The kernels scan piece counts in tiles of TILE elements, 16 tiles to a k_reduce workgroup, and the ticket winner's carry loop
runs once per 256 workgroups (2^20 elements).  k_expand writes output tiles of OUT_TILE items from at most 10 source tiles;
k_path_spans reads the tile prefixes at path boundaries; spans that do not tile the steps pool go to k_path_lens /
k_expand_paths, one workgroup per path and one 256-step chunk at a time.  Each generator below puts counts, boundaries or
totals at those edges.

A Shape's expected result comes from chop_model.chop_fast (chop_model.chop at the reduced sizes tests/test_chop_model.py
uses); F and G carry closed forms in Python ints instead, G's as a function of a chunk of positions that evaluates on numpy
or torch int64 arrays alike, so 2^32 items are checked on the device without ever being on the host.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

from oracle import flatgfa_oracle as fo

TILE, TILES_PER_WG, OUT_TILE = 256, 16, 2048
WG_ELEMS = TILE * TILES_PER_WG  # 4096
CARRY = 256 * WG_ELEMS  # 2^20: more elements than this and the carry loop of k_reduce runs more than once
SCAN_FULL = (1, 255, 256, 257, 4095, 4096, 4097, CARRY, CARRY + 1, CARRY + 4097, 3 * CARRY + 5)
SCAN_SMALL = SCAN_FULL[:7]
ERR_BOUNDS, ERR_TOO_LARGE = -2, -6
C = 3  # the cut of the A-E shapes: lengths 0..12 make 1 to 4 pieces


class Shape(NamedTuple):
    name: str
    pools: fo.Pools
    c: int
    err: Optional[int] = None  # the code of the device entry and of FlatGFA.chop without links (None: success)
    err_links: Optional[int] = None  # the code of FlatGFA.chop with links
    host: bool = True  # also a valid input to FlatGFA.chop (its spans lie inside the pool)


def tiles(p: fo.Pools) -> bool:
    """k_check_spans' verdict: the spans tile the steps pool in order (no path at all does not)."""
    b, e = p.paths["steps_start"].astype(np.int64), p.paths["steps_end"].astype(np.int64)
    return bool(len(b) and b[0] == 0 and np.array_equal(b[1:], e[:-1]) and e[-1] == len(p.steps))


def pieces(n: int, c: int) -> int:
    return 1 if n <= c else (n - 1) // c + 1


def make_pools(lens, steps, spans, links=(), seq=True) -> fo.Pools:
    """Segments of `lens` laid out one after another in seq_data (or all at offset 0 when seq is False), named 1..S; paths
    with the given (begin, end) spans, all named "p"; links as (from handle, to handle)."""
    lens = np.asarray(lens, dtype=np.int64)
    S = len(lens)
    segs = np.zeros(S, fo.SEG_DT)
    segs["name"] = np.arange(1, S + 1)
    if seq:
        st = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        segs["seq_start"], segs["seq_end"] = st, st + lens
        seq_data = np.full(int(lens.sum()), ord("A"), np.uint8)
    else:
        segs["seq_end"] = lens
        seq_data = np.zeros(0, np.uint8)
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    paths = np.zeros(len(spans), fo.PATH_DT)
    paths["name_end"] = 1
    paths["steps_start"], paths["steps_end"] = spans[:, 0], spans[:, 1]
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    lk = np.zeros(len(links), fo.LINK_DT)
    lk["from_"], lk["to"] = links[:, 0], links[:, 1]
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=paths, links=lk, steps=np.asarray(steps, dtype=np.uint32), seq_data=seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(b"p", np.uint8).copy(),
                    optional_data=z, line_order=z)


def mixed_lens(rng, n, c=C):
    """Lengths 0..4c: a mix of 1-piece and 2- to 4-piece segments."""
    return rng.integers(0, 4 * c + 1, n)


def handles(rng, segs):
    segs = np.asarray(segs, dtype=np.int64)
    return ((segs << 1) | rng.integers(0, 2, len(segs))).astype(np.uint32)


def random_links(rng, S, n=40):
    return np.stack([handles(rng, rng.integers(0, S, n)), handles(rng, rng.integers(0, S, n))], axis=1) if S else np.zeros((0, 2))


def tiling_spans(rng, n, n_paths):
    """n_paths spans that tile [0, n) in order (some empty)."""
    cuts = np.sort(rng.integers(0, n + 1, n_paths - 1))
    b = np.concatenate([[0], cuts])
    return np.stack([b, np.concatenate([cuts, [n]])], axis=1)


# ---- A. scan edges: counts at 1, tile and workgroup edges, and past 2^20 ----
def a_segs(n: int, seed: int = 0) -> Shape:
    """n segments (one tiling path over up to 4097 steps that reach the first, last and some middle segments)."""
    rng = np.random.default_rng(seed)
    lens = mixed_lens(rng, n)
    ids = np.concatenate([[0, n - 1], rng.integers(0, n, min(n, 4097))])
    steps = handles(rng, ids)
    return Shape(f"A_segs_{n}", make_pools(lens, steps, tiling_spans(rng, len(steps), 2), random_links(rng, n)), C)


def a_steps(n: int, seed: int = 0) -> Shape:
    """n steps over 300 segments, in up to 7 tiling paths."""
    rng = np.random.default_rng(seed + 1)
    steps = handles(rng, rng.integers(0, 300, n))
    return Shape(f"A_steps_{n}", make_pools(mixed_lens(rng, 300), steps, tiling_spans(rng, n, min(n, 7)), random_links(rng, 300)), C)


def a_paths(n: int, seed: int = 0) -> Shape:
    """n paths in non-tiling layout: path p spans [p + 1, p + 1 + w) with w in 1..2 over n + 2 steps (the first path leaves
    step 0 out; no path is empty, so the GFA printer takes them all), so the per-path scan runs over n elements."""
    rng = np.random.default_rng(seed + 2)
    steps = handles(rng, rng.integers(0, 300, n + 2))
    b = np.arange(1, n + 1)
    e = b + rng.integers(1, 3, n)
    return Shape(f"A_paths_{n}", make_pools(mixed_lens(rng, 300), steps, np.stack([b, e], axis=1), random_links(rng, 300)), C)


def shapes_a(counts=SCAN_FULL) -> List[Shape]:
    return [f(n) for n in counts for f in (a_segs, a_steps, a_paths)]


# ---- B. output-tile edges ----
def _fill_to(k, total):
    """The prefix of the piece counts k that stays within total, and how many 1-piece elements make up the rest."""
    keep = int(np.searchsorted(np.cumsum(k), total, side="right"))
    return keep, total - int(np.sum(k[:keep]))


def b_seg_total(total: int, seed: int = 0) -> Shape:
    """Segments whose pieces add up to exactly total (S' = total)."""
    rng = np.random.default_rng(seed + 3)
    lens = mixed_lens(rng, total)
    keep, rest = _fill_to(np.array([pieces(int(x), C) for x in lens]), total)
    lens = np.concatenate([lens[:keep], np.ones(rest, np.int64)])
    rng.shuffle(lens)
    S = len(lens)
    steps = handles(rng, rng.integers(0, S, 600))
    return Shape(f"B_S2_{total}", make_pools(lens, steps, tiling_spans(rng, 600, 3)), C)


def b_step_total(total: int, tiling: bool, seed: int = 0) -> Shape:
    """Steps whose pieces add up to exactly total (N' = total), in three tiling paths or in one path with a trailing
    unused step (non-tiling)."""
    rng = np.random.default_rng(seed + 4)
    lens = np.concatenate([[1], mixed_lens(rng, 299)])  # segment 0 is 1 piece
    k = np.array([pieces(int(x), C) for x in lens])
    ids = rng.integers(0, 300, total)
    keep, rest = _fill_to(k[ids], total)
    ids = np.concatenate([ids[:keep], np.zeros(rest, np.int64)])
    rng.shuffle(ids)
    n = len(ids)
    steps = handles(rng, ids)
    if tiling:
        spans = tiling_spans(rng, n, 3)
    else:
        steps, spans = np.concatenate([steps, handles(rng, [5])]), [(0, n)]
    return Shape(f"B_N2_{total}_{'tiling' if tiling else 'paths'}", make_pools(lens, steps, spans), C)


def b_nine_tiles(as_steps: bool, seed: int = 0) -> Shape:
    """The first element has 2 pieces and every other 1: output tile o starts on the last element of source tile 8o - 1 and
    needs the 9 source tiles 8o - 1 .. 8o + 7 (k_expand's kRMax)."""
    rng = np.random.default_rng(seed + 5)
    n = 5 * OUT_TILE + 300
    if not as_steps:
        lens = np.concatenate([[C + 1], rng.integers(0, C + 1, n - 1)])
        return Shape("B_nine_tiles_segs", make_pools(lens, handles(rng, rng.integers(0, n, 500)), tiling_spans(rng, 500, 2)), C)
    lens = np.concatenate([[2 * C], rng.integers(0, C + 1, 299)])
    steps = handles(rng, np.concatenate([[0], rng.integers(1, 300, n - 1)]))
    return Shape("B_nine_tiles_steps", make_pools(lens, steps, tiling_spans(rng, n, 4)), C)


def b_whole_tiles(m: int, lead: int, as_steps: bool, seed: int = 0) -> Shape:
    """One element of 2048 m pieces (len = 2048 m c) after `lead` 1-piece elements: with lead = 0 it fills m output tiles
    exactly, with lead = 1000 it starts in the middle of one."""
    rng = np.random.default_rng(seed + 6)
    big = OUT_TILE * m * C
    tail = rng.integers(0, 4 * C + 1, 500)
    if not as_steps:
        lens = np.concatenate([rng.integers(0, C + 1, lead), [big], tail])
        ids = np.concatenate([[lead], rng.integers(0, len(lens), 300)])
        return Shape(f"B_whole_{m}_{lead}_segs", make_pools(lens, handles(rng, ids), tiling_spans(rng, len(ids), 2)), C)
    lens = np.concatenate([[big, 1], rng.integers(0, 4 * C + 1, 298)])
    ids = np.concatenate([np.ones(lead, np.int64), [0], rng.integers(1, 300, 700), [0]])
    return Shape(f"B_whole_{m}_{lead}_steps", make_pools(lens, handles(rng, ids), tiling_spans(rng, len(ids), 3)), C)


def shapes_b(m: int = 3) -> List[Shape]:
    out = []
    for t in (OUT_TILE * m - 1, OUT_TILE * m, OUT_TILE * m + 1):
        out += [b_seg_total(t), b_step_total(t, True), b_step_total(t, False)]
    out += [b_nine_tiles(False), b_nine_tiles(True)]
    for lead in (0, 1000):
        out += [b_whole_tiles(m, lead, False), b_whole_tiles(m, lead, True)]
    return out


# ---- C. tiling spans at tile edges ----
def c_edges(n_tiles: int, rem: int, seed: int = 0) -> Shape:
    """Path boundaries at every 256 k - 1, 256 k, 256 k + 1, with empty paths at 0, at 512 and at n_steps; n_steps =
    256 n_tiles + rem (rem = 0: k_path_spans reads prefix[n_tiles] for the last end)."""
    rng = np.random.default_rng(seed + 7)
    n = TILE * n_tiles + rem
    inner = sorted(x for x in {TILE * k + d for k in range(1, n_tiles + 1) for d in (-1, 0, 1)} if 0 < x < n)
    cuts = sorted([0, 0] + inner + [n, n] + ([2 * TILE] if 2 * TILE in inner else []))  # (the doubled ones: empty paths)
    spans = list(zip(cuts[:-1], cuts[1:]))
    steps = handles(rng, rng.integers(0, 300, n))
    return Shape(f"C_edges_{n_tiles}_{rem}", make_pools(mixed_lens(rng, 300), steps, spans), C)


def c_many_paths(n_paths: int, seed: int = 0) -> Shape:
    """Many short tiling paths (0 to 3 steps): far more paths than k_path_spans has waves in a block."""
    rng = np.random.default_rng(seed + 8)
    w = rng.integers(0, 4, n_paths)
    e = np.cumsum(w)
    spans = np.stack([e - w, e], axis=1)
    steps = handles(rng, rng.integers(0, 300, int(e[-1])))
    return Shape(f"C_many_{n_paths}", make_pools(mixed_lens(rng, 300), steps, spans), C)


def shapes_c() -> List[Shape]:
    return [c_edges(12, 0), c_edges(12, 1), c_edges(12, 255), c_edges(1, 0), c_many_paths(1000), c_many_paths(70_001)]


# ---- D. non-tiling spans, one trigger at a time, and per-path chunks at output-tile edges ----
def _d_base(seed):
    rng = np.random.default_rng(seed + 9)
    n = 2000
    spans = np.array([(0, 300), (300, 555), (555, 556), (556, 1000), (1000, 1000), (1000, 1513), (1513, 1800), (1800, n)])
    return rng, mixed_lens(rng, 300), handles(rng, rng.integers(0, 300, n)), spans


def d_trigger(kind: str, seed: int = 0) -> Shape:
    rng, lens, steps, spans = _d_base(seed)
    if kind == "gap_first":
        spans[0, 0] = 5
    elif kind == "gap_between":
        spans[3, 0] += 3
    elif kind == "trailing":
        spans[-1, 1] -= 3
    elif kind == "swapped":
        spans[[3, 5]] = spans[[5, 3]]
    elif kind == "repeated":
        spans = np.insert(spans, 4, spans[3], axis=0)
    elif kind == "no_paths":
        spans = spans[:0]
    return Shape(f"D_{kind}", make_pools(lens, steps, spans, random_links(rng, 300)), C)


D_TRIGGERS = ("gap_first", "gap_between", "trailing", "swapped", "repeated", "no_paths")


def d_chunk(total: int, seed: int = 0) -> Shape:
    """One path over exactly one 256-step chunk (from step 1, so non-tiling) whose pieces add up to total."""
    rng = np.random.default_rng(seed + 10)
    q, r = divmod(total, TILE)
    kmax = q + 2
    # segment k - 1 has k pieces, its length anywhere in ((k - 1) c, k c]
    lens = np.array([rng.integers((k - 1) * C + 1, k * C + 1) if k > 1 else rng.integers(0, C + 1) for k in range(1, kmax + 1)])
    ks = np.array([q + 1] * r + [q] * (TILE - r))
    rng.shuffle(ks)
    steps = handles(rng, np.concatenate([[3], ks - 1, [4]]))
    return Shape(f"D_chunk_{total}", make_pools(lens, steps, [(1, TILE + 1)]), C)


def d_long_path(n: int, seed: int = 0) -> Shape:
    """Two long non-tiling paths (many 256-step chunks each), the second over the first's steps again."""
    rng = np.random.default_rng(seed + 11)
    steps = handles(rng, rng.integers(0, 300, n))
    return Shape(f"D_long_{n}", make_pools(mixed_lens(rng, 300), steps, [(7, n - 2), (0, n // 2 + 1)]), C)


def shapes_d(m: int = 3) -> List[Shape]:
    out = [d_trigger(k) for k in D_TRIGGERS]
    out += [d_chunk(t) for t in (OUT_TILE * m - 1, OUT_TILE * m, OUT_TILE * m + 1)]
    out += [d_long_path(100_003), a_paths(5000, seed=5)]
    return out


# ---- E. errors and what is not an error ----
def shapes_e() -> List[Shape]:
    rng, lens, steps, spans = _d_base(0)
    S = len(lens)
    out = []
    # an out-of-range step where no path walks (a gap, the unused tail) is not an error: chop.rs walks only the paths
    gap, inside = int(spans[3, 0]) + 1, 1200
    s1, sp1 = steps.copy(), spans.copy()
    sp1[3, 0] += 3
    s1[gap] = (S + 5) << 1
    sp1[-1, 1] -= 3
    s1[-1] = 0xFFFFFFFF
    out.append(Shape("E_bad_step_in_gap", make_pools(lens, s1, sp1), C))
    # the same step inside a span, in tiling and non-tiling layouts
    s2 = steps.copy()
    s2[inside] = (S + 5) << 1
    out.append(Shape("E_bad_step_tiling", make_pools(lens, s2, spans), C, ERR_BOUNDS, ERR_BOUNDS))
    s2[-1] = 0xFFFFFFFF
    out.append(Shape("E_bad_step_paths", make_pools(lens, s2, sp1), C, ERR_BOUNDS, ERR_BOUNDS))
    s3 = steps.copy()
    s3[-1] = (S << 1) | 1  # (the first id past the end, in the last tile)
    out.append(Shape("E_bad_step_last", make_pools(lens, s3, spans), C, ERR_BOUNDS, ERR_BOUNDS))
    # spans outside the pool (the device entry only: FlatGFA's loader checks spans)
    sp4 = spans.copy()
    sp4[-1, 1] = len(steps) + 1
    out.append(Shape("E_span_past_end", make_pools(lens, steps, sp4), C, ERR_BOUNDS, ERR_BOUNDS, host=False))
    sp5 = spans.copy()
    sp5[2] = (600, 599)
    out.append(Shape("E_span_reversed", make_pools(lens, steps, sp5), C, ERR_BOUNDS, ERR_BOUNDS, host=False))
    # a link past the segments: an error with links, not looked at without
    lk = random_links(rng, S)
    lk[7, 1] = (S << 1) | 1
    full = spans[spans[:, 0] < spans[:, 1]]  # (no empty path: this one goes through the GFA printer and parser)
    out.append(Shape("E_bad_link", make_pools(lens, steps, full, lk), C, None, ERR_BOUNDS))
    return out


def catalog(full: bool = True) -> List[Tuple[str, Callable[[], Shape], bool, bool]]:
    """(name, factory, tiling, host) of every A-E shape; the A shapes are built only when called."""
    out = []
    for n in (SCAN_FULL if full else SCAN_SMALL):
        out += [(f"A_segs_{n}", lambda n=n: a_segs(n), True, True), (f"A_steps_{n}", lambda n=n: a_steps(n), True, True),
                (f"A_paths_{n}", lambda n=n: a_paths(n), False, True)]
    for f in (shapes_b, shapes_c, shapes_d, shapes_e):
        out += [(s.name, lambda s=s: s, tiles(s.pools), s.host) for s in f()]
    return out


# ---- F. u64 length and c arithmetic (the device entry: seg_len only) ----
F_LENS = (0, 1, 2**31, 2**32 - 2, 2**32 - 1)
F_CS = (1, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**40, 2**63)


def f_lens(c: int):
    return F_LENS[:2] if c == 1 else F_LENS


def f_shape(c: int) -> Shape:
    """One segment of each length in F_LENS (0 and 1 only at c = 1), stepped forward then backward by one path."""
    lens = f_lens(c)
    steps = [h for s in range(len(lens)) for h in (s << 1, (s << 1) | 1)]
    return Shape(f"F_c{c}", make_pools(lens, steps, [(0, len(steps))], seq=False), c, host=False)


def f_expect(lens, c: int):
    """(seg_first, new lengths, new steps) of f_shape's graph, in Python ints."""
    first, new_len, steps = [0], [], []
    for n in lens:
        k = pieces(n, c)
        new_len += [c] * (k - 1) + [n - (k - 1) * c]
        first.append(first[-1] + k)
    for s in range(len(lens)):
        ids = range(first[s], first[s + 1])
        steps += [i << 1 for i in ids] + [(i << 1) | 1 for i in reversed(ids)]
    return first, new_len, steps


# ---- G. the 32-bit limits, in closed form ----
class Limit:
    """Segments A (length la) and B (length 1); one path A+, A-, then n_b steps B+; with trailing, one more B+ that no path
    walks (so the spans do not tile the pool).  At la = 2^31 - 2, c = 1: S' = 2^31 - 1 and N' = 2^32 - 1 with n_b = 3."""

    def __init__(self, la: int, n_b: int, c: int, trailing: bool):
        self.la, self.n_b, self.c, self.trailing = la, n_b, c, trailing
        self.ka = pieces(la, c)
        self.S2 = self.ka + 1
        self.N2 = 2 * self.ka + n_b

    def arrays(self):
        """(steps, path_begin, path_end, n_segs, seg_len) of the input, as numpy arrays."""
        n = 2 + self.n_b
        steps = np.array([0, 1] + [2] * (self.n_b + int(self.trailing)), np.uint32)
        return steps, np.array([0], np.uint32), np.array([n], np.uint32), 2, np.array([self.la, 1], np.uint32)

    def pools(self) -> fo.Pools:
        steps, b, e, _, lens = self.arrays()
        return make_pools(lens, steps, [(int(b[0]), int(e[0]))])

    def seg_first(self):
        return [0, self.ka, self.ka + 1]

    def steps_at(self, j):
        """The new step handles at positions j (an int64 numpy array or torch tensor)."""
        ka = self.ka
        fwd, bwd = j < ka, (j >= ka) & (j < 2 * ka)
        return fwd * (j << 1) + bwd * (((2 * ka - 1 - j) << 1) | 1) + (j >= 2 * ka) * (ka << 1)

    def seg_len_at(self, i):
        """The new segment lengths at ids i (an int64 numpy array or torch tensor)."""
        ka, c = self.ka, self.c
        return (i < ka - 1) * c + (i == ka - 1) * (self.la - (ka - 1) * c) + (i == ka) * 1


LIMIT_LA = 2**31 - 2
LIMIT_OK = [Limit(LIMIT_LA, 3, 1, t) for t in (False, True)]  # S' = 2^31 - 1, N' = 2^32 - 1: accepted
LIMIT_N2 = [Limit(LIMIT_LA, 4, 1, t) for t in (False, True)]  # N' = 2^32: refused


def limit_s2_refused():
    """One segment of length 2^31 at c = 1, stepped once: S' = 2^31, refused.  (steps, begin, end, n_segs, seg_len)"""
    return np.array([0], np.uint32), np.array([0], np.uint32), np.array([1], np.uint32), 1, np.array([2**31], np.uint32)
