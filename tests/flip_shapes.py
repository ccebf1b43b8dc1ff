"""Builders of small graphs for the flip tests, and the smallest ones at which each seam of the flip kernels
(pollen_amd/csrc/flip_device.hip) can break: tiles of T laid-out steps, waves of 64, rows of the key table at the two
thresholds between the wave's, the LDS and the in-place sort, the scans' tiles, and input spans that are not the paths one
behind another.  SHAPES maps a name to a function that makes the pools; tests/test_flip_model.py holds the model's two forms
of the de-duplication to each other on every shape, tests/test_gpu_flip_geometry.py runs them on the device."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import flip_model as fm
from oracle import flatgfa_oracle as fo

T = fm.TILE
LinkSpec = Tuple[int, int, Sequence[int]]  # from, to, the overlap's ops


def h(seg: int, back: bool = False) -> int:
    return (seg << 1) | (1 if back else 0)


def graph(seg_lens: Sequence[int], paths: Sequence[Sequence[int]], links: Sequence[LinkSpec] = (), names: Optional[List[bytes]] = None,
          spans: Optional[Sequence[Tuple[int, int]]] = None, steps: Optional[np.ndarray] = None) -> fo.Pools:
    """Pools of segments of these lengths (named 1.., their bases A), paths of these handles (named p0.. unless `names`), links
    with these overlaps.  spans and steps: the step pool and the paths' spans in it, where they are not the paths one behind
    another."""
    lens = np.asarray(seg_lens, dtype=np.int64)
    end = np.cumsum(lens)
    segs = np.zeros(len(lens), fo.SEG_DT)
    if len(lens):
        segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, len(lens) + 1), end - lens, end
    if steps is None:
        arrs = [np.asarray(p, dtype=np.uint32) for p in paths]
        steps = np.concatenate(arrs) if arrs else np.zeros(0, np.uint32)
        e = np.cumsum([len(a) for a in arrs], dtype=np.int64)
        spans = [(int(e[i]) - len(a), int(e[i])) for i, a in enumerate(arrs)]
    names = names if names is not None else [b"p%d" % i for i in range(len(spans))]
    rec = np.zeros(len(spans), fo.PATH_DT)
    n_end = np.cumsum([len(n) for n in names], dtype=np.int64)
    for i, (a, b) in enumerate(spans):
        rec[i] = (int(n_end[i]) - len(names[i]), int(n_end[i]), a, b, 0, 0)
    al: List[int] = []
    lk = np.zeros(len(links), fo.LINK_DT)
    for i, (f, t, ops) in enumerate(links):
        lk[i] = (f, t, len(al), len(al) + len(ops))
        al += list(ops)
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=rec, links=lk, steps=np.asarray(steps, dtype=np.uint32), seq_data=np.full(int(lens.sum()), 65, np.uint8),
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.asarray(al, dtype=np.uint32), name_data=np.frombuffer(b"".join(names), np.uint8).copy(),
                    optional_data=z, line_order=z)


def op(n: int, code: int = 0) -> int:
    """One alignment op: code 0 M, 1 N, 2 D, 3 I (flatgfa_core.hpp), length above the low byte."""
    return (n << 8) | code


def walk(n: int, n_segs: int, seed: int, back: float) -> np.ndarray:
    """n random steps over n_segs segments, a share `back` of them backward."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, n_segs, n) << 1) | (rng.random(n) < back)).astype(np.uint32)


def lengths(n_segs: int = 40, seed: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).integers(1, 30, n_segs)


def some_links(n_segs: int, n: int, seed: int) -> List[LinkSpec]:
    rng = np.random.default_rng(seed)
    out: List[LinkSpec] = []
    for _ in range(n):
        f, t = int(rng.integers(0, 2 * n_segs)), int(rng.integers(0, 2 * n_segs))
        out.append((f, t, [[op(0)], [op(5)], [op(3), op(1, 2)], []][int(rng.integers(0, 4))]))
    out += out[: n // 4]                                     # verbatim
    out += [(t ^ 1, f ^ 1, ops) for f, t, ops in out[: n // 4]]  # as their reverses
    return out


def of_lengths(ns: Sequence[int], backs: Sequence[float], n_links: int = 30) -> fo.Pools:
    """Paths of these many steps, path k with a share backs[k % len(backs)] of backward steps."""
    return graph(lengths(), [walk(n, 40, 7 + k, backs[k % len(backs)]) for k, n in enumerate(ns)], some_links(40, n_links, 5))


def not_laid_out() -> fo.Pools:
    """Spans that leave gaps, overlap, repeat and run against the path order, over one step pool."""
    pool = walk(3 * T, 40, 11, 0.5)
    spans = [(2 * T + 5, 3 * T), (10, 700), (300, 1200), (300, 1200), (T - 3, T + 3), (0, 0), (T + 50, 2 * T + 60), (5, 6)]
    return graph(lengths(), [], some_links(40, 20, 6), spans=spans, steps=pool)


def row_of(n0: int) -> fo.Pools:
    """Rows of n0 and n0 - 2 keys.  One turned path whose new steps are 0+, k1+, 0+, k2+, .. kr+, r = n0 - 3: r candidates with
    the high handle 0+ (the pairs 0+ -> k) and r - 1 with the high handle 0- (the pairs k -> 0+, as their reverses), every
    tenth k a repeat; and old links in both rows, three and two, with and without a candidate's pair and overlap."""
    r = n0 - 3
    ks = np.arange(1, r + 1)
    ks[9::10] = ks[8::10][: len(ks[9::10])]
    new = np.zeros(2 * r, np.uint32)
    new[1::2] = ks << 1
    links = [(h(0), h(3), [op(0)]), (h(0), h(4), [op(5)]), (h(5, True), h(0, True), [op(0)]), (h(6), h(0), [op(0)]), (h(6), h(0), [op(2)])]
    return graph(np.ones(r + 1, np.int64), [(new[::-1] ^ 1)], links)


def repeated_pair(n: int) -> fo.Pools:
    """A turned path that walks one pair n times: n + 1 backward steps of one segment."""
    return graph([3, 2], [np.full(n + 1, h(1, True), np.uint32), [h(0), h(1)]], [(h(0), h(1), [op(0)])])


def heavy(fwd_steps: int, back_steps: int) -> fo.Pools:
    """One segment of 2^16 bases, stepped forward and backward this often (interleaved, so that every tile holds both)."""
    n, fewer = fwd_steps + back_steps, min(fwd_steps, back_steps)
    st = np.full(n, 1 if back_steps > fwd_steps else 0, np.uint32)
    st[np.linspace(0, n - 1, fewer).astype(np.int64)] ^= 1
    assert int(st.sum()) == back_steps
    return graph([1 << 16], [st, [0, 1, 1]])


SHAPES: Dict[str, Callable[[], fo.Pools]] = {
    "paths of T-1, T, T+1, 2T+1 steps, turned": lambda: of_lengths([T - 1, T, T + 1, 2 * T + 1], [0.9]),
    "paths of T-1, T, T+1, 2T+1 steps, every other turned": lambda: of_lengths([T - 1, T, T + 1, 2 * T + 1], [0.9, 0.1]),
    "a turned path that begins and ends mid-tile": lambda: of_lengths([100, T, 300], [0.1, 0.9, 0.1]),
    "a turned path over three tiles between two that stay": lambda: of_lengths([T // 2, 2 * T + T // 2, 77], [0.1, 0.9, 0.1]),
    "many whole paths in one tile": lambda: of_lengths([5] * 300 + [3] * 200, [0.9, 0.1, 0.5]),
    "paths of 0, 1 and 2 steps between long ones": lambda: of_lengths([T + 9, 0, 1, 2, 0, 0, T, 1, 0, 2 * T, 2, 0], [0.9, 0.9, 0.9, 0.9, 0.1]),
    "only empty paths": lambda: of_lengths([0, 0, 0], [0.9]),
    "no paths": lambda: graph(lengths(), [], some_links(40, 12, 3)),
    "no links": lambda: graph(lengths(), [walk(50, 40, 1, 0.9), walk(50, 40, 2, 0.1)]),
    "no paths and no links": lambda: graph([1, 2], []),
    "paths of empty segments": lambda: graph([0, 0, 5], [[h(0, True), h(1, True)], [h(2, True), h(0)]]),
    "gapped, overlapping and out-of-order spans": not_laid_out,
    **{"rows of SHORT%+d and SHORT%+d keys" % (d, d - 2): (lambda d=d: row_of(fm.SHORT_ROW + d)) for d in (-1, 0, 1, 2, 3)},
    **{"rows of LDS%+d and LDS%+d keys" % (d, d - 2): (lambda d=d: row_of(fm.LDS_ROW + d)) for d in (-1, 0, 1, 2, 3)},
    "one pair 10^5 times": lambda: repeated_pair(100000),
    "scan tile - 1 paths": lambda: of_lengths([3] * (fm.SCAN_TILE - 1), [0.9, 0.1]),
    "scan tile paths": lambda: of_lengths([3] * fm.SCAN_TILE, [0.9, 0.1]),
    "scan tile + 1 paths": lambda: of_lengths([3] * (fm.SCAN_TILE + 1), [0.9, 0.1]),
    "links past a scan tile": lambda: of_lengths([40, 50], [0.9, 0.1], n_links=fm.SCAN_TILE),
}

# Only 64-bit sums get these right: fwd = 2^32 + 2^16 against rev = 2^31 stays (a sum that wraps at 2^32 sees 2^16 < 2^31 and
# turns it), and the mirror turns (a wrapped sum would leave it).
HEAVY = {"fwd 2^32+2^16, rev 2^31": lambda: heavy((1 << 16) + 1, 1 << 15), "rev 2^32+2^16, fwd 2^31": lambda: heavy(1 << 15, (1 << 16) + 1)}
