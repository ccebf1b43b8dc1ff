"""Path depth (flatgfa/src/ops/depth.rs:88-131) restated on the structure-of-arrays image (steps, path_begin, path_end,
seg_len), for the tests only: exact integers, no fixed width anywhere.

  depth[s]        the number of steps on segment s, over all paths (depth.rs:45-56)
  length[p]       sum of seg_len over path p's steps                (depth.rs:125)
  weighted[p]     sum of depth * seg_len over them                  (depth.rs:124)
  mean[p]         weighted as f64 / length as f64                   (depth.rs:129)

Rust's `as f64` converts an integer to the nearest binary64, ties to even; Python's float(int) does the same (and raises
beyond the format's range, which 2^64 - 1 is far from), so mean_of() below is float(weighted) / float(length).  0 / 0 is the
NaN the hardware's division makes -- numpy's division, not Python's ZeroDivisionError and not float("nan"), whose sign
differs -- and the tests compare it bitwise.

Next to the answers the model reports the intermediate values the kernels hold (depth_accum.hip: block_scan's LW table,
sum_groups' records and lane shares, k_path_reduce's per-window partials; depth_device.hip: k_path_sums' thread, wave and
block sums), so that tests/path_depth_shapes.py can prove on the CPU that a shape carries into the upper word where it
says it does.  `Twin` is the same in wrapping uint64 for the larger shapes; it is checked against the exact model wherever
that is affordable and asserts the precondition of every shape: all totals below 2^64 (where the reference's usize wraps in
a release build and panics in a debug one).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np

TWO32 = 1 << 32
TWO64 = 1 << 64


def mean_of(length: int, weighted: int) -> np.float64:
    """(weighted as f64) / (length as f64): each total rounded to nearest-even once, then one division."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide(np.float64(float(weighted)), np.float64(float(length)))


def means(length, weighted) -> np.ndarray:
    return np.array([mean_of(int(l), int(w)) for l, w in zip(length, weighted)], np.float64)


def seg_depth(steps, n_segs: int, path_begin, path_end) -> np.ndarray:
    """depth.rs:45-56 over the paths' spans (steps outside every span count for nothing; overlapping spans count twice)."""
    d = np.zeros(n_segs, np.int64)
    ids = np.asarray(steps, np.uint32) >> 1
    for b, e in zip(path_begin, path_end):
        d += np.bincount(ids[int(b):int(e)], minlength=n_segs)
    return d


class Answer(NamedTuple):
    length: List[int]
    weighted: List[int]
    mean: np.ndarray  # float64[P]
    depth: np.ndarray  # int64[S]


def exact(steps, path_begin, path_end, seg_len, n_segs: int) -> Answer:
    """The reference's loop, in Python ints."""
    d = seg_depth(steps, n_segs, path_begin, path_end)
    ids = np.asarray(steps, np.uint32) >> 1
    lens = np.asarray(seg_len, np.uint32).astype(object)
    wl = lens * d.astype(object)
    length, weighted = [], []
    for b, e in zip(path_begin, path_end):
        s = ids[int(b):int(e)]
        length.append(int(lens[s].sum()) if len(s) else 0)
        weighted.append(int(wl[s].sum()) if len(s) else 0)
    return Answer(length, weighted, means(length, weighted), d)


def window_bits(n_segs: int) -> int:
    """depth_fast.hip: 4096-segment windows, 8192 above 4 Mi segments."""
    return 13 if n_segs > (4 << 20) else 12


# ---- what the kernels hold on the way, exact ----
def window_prefix(seg_len, depth, n_segs: int, wb: int, win: int) -> Tuple[List[int], List[int]]:
    """LW of window `win`: LW[i] = the sums over the window's first i segments (i = 0 .. nvalid) of seg_len and of
    depth * seg_len -- what block_scan<unsigned long long, kPer> leaves in LDS."""
    lo, hi = win << wb, min(n_segs, (win + 1) << wb)
    L, Wt = [0], [0]
    for s in range(lo, hi):
        L.append(L[-1] + int(seg_len[s]))
        Wt.append(Wt[-1] + int(depth[s]) * int(seg_len[s]))
    return L, Wt


class Run(NamedTuple):
    path: int
    piece: int  # which piece of its path (0 when paths are not cut)
    win: int
    first: int  # the run's first segment
    n: int  # segments in the record: 1 .. run_cap
    length: int
    weighted: int


def runs(steps, path_begin, path_end, seg_len, depth, wb: int, run_cap: int = 1024, piece_steps: int = 0) -> List[Run]:
    """The run records of an in-order scan: maximal stretches of steps whose segment ids go up by one, inside one path (or
    one piece of `piece_steps` steps of it), cut where the next segment begins a window and after `run_cap` segments (the
    record's length field: sum_groups' (rec >> WB) & 1023, plus one).  The kernel may cut a run finer (at the edges of its
    1024-step blocks) and takes a descending stretch from its low end as one record; the shapes that claim something of a
    single record begin it at its path's first step and let it ascend."""
    ids = (np.asarray(steps, np.uint32) >> 1).astype(np.int64)
    out = []
    for p, (b, e) in enumerate(zip(path_begin, path_end)):
        b, e = int(b), int(e)
        i = b
        while i < e:
            j = i + 1
            piece = (i - b) // piece_steps if piece_steps else 0
            stop = min(e, b + (piece + 1) * piece_steps) if piece_steps else e
            while j < stop and ids[j] == ids[j - 1] + 1 and (ids[j] & ((1 << wb) - 1)) != 0 and j - i < run_cap:
                j += 1
            segs = ids[i:j]
            out.append(Run(p, piece, int(ids[i]) >> wb, int(ids[i]), j - i, sum(int(seg_len[s]) for s in segs),
                           sum(int(depth[s]) * int(seg_len[s]) for s in segs)))
            i = j
    return out


def item_partials(rs: List[Run]) -> Dict[Tuple[int, int, int], Tuple[int, int]]:
    """(path, piece, window) -> the sums sum_groups stores for that item in that window (psum_part)."""
    out: Dict[Tuple[int, int, int], Tuple[int, int]] = {}
    for r in rs:
        l, w = out.get((r.path, r.piece, r.win), (0, 0))
        out[(r.path, r.piece, r.win)] = (l + r.length, w + r.weighted)
    return out


def lane_shares(rs: List[Run], path: int, piece: int, win: int) -> List[Tuple[int, int]]:
    """The 64 lanes' shares of one item's sums in one window: lane i adds the item's records i, i + 64, ... there."""
    mine = [r for r in rs if (r.path, r.piece, r.win) == (path, piece, win)]
    sh = [[0, 0] for _ in range(64)]
    for k, r in enumerate(mine):
        sh[k % 64][0] += r.length
        sh[k % 64][1] += r.weighted
    return [tuple(x) for x in sh]


# ---- the gather kernel's geometry (depth_device.hip: k_path_sums, path_sums_launch) ----
def split_of(n_ids: int, n_cus: int) -> int:
    return max(1, min(64, (16 * n_cus) // n_ids))


class Gather(NamedTuple):
    threads: List[Tuple[int, int]]  # per thread: (length, weighted)
    waves: List[Tuple[int, int]]
    block: Tuple[int, int]
    n_batches: int  # trips of the eight-deep loop of thread 0
    n_tail: int  # trips of its one-step tail loop


def gather_slice(steps, begin: int, end: int, seg_len, depth, split: int, part: int, sum_threads: int = 256, batch: int = 8) -> Gather:
    """One block of k_path_sums: slice `part` of `split` of the path [begin, end)."""
    n = end - begin
    lo, hi = begin + n * part // split, begin + n * (part + 1) // split
    ids = np.asarray(steps[lo:hi], np.uint32) >> 1
    th = []
    for t in range(sum_threads):
        s = ids[t::sum_threads]
        th.append((sum(int(seg_len[x]) for x in s), sum(int(depth[x]) * int(seg_len[x]) for x in s)))
    wv = [(sum(a for a, _ in th[w:w + 64]), sum(c for _, c in th[w:w + 64])) for w in range(0, sum_threads, 64)]
    i, nb, nt = lo, 0, 0  # thread 0's loop trips
    while i + (batch - 1) * sum_threads < hi:
        i += batch * sum_threads
        nb += 1
    while i < hi:
        i += sum_threads
        nt += 1
    return Gather(th, wv, (sum(a for a, _ in wv), sum(c for _, c in wv)), nb, nt)


# ---- the uint64 twin ----
class Twin(NamedTuple):
    length: np.ndarray  # uint64[P]
    weighted: np.ndarray
    mean: np.ndarray
    depth: np.ndarray


def twin(steps, path_begin, path_end, seg_len, n_segs: int) -> Twin:
    """The same sums in uint64, vectorised.  Asserts what every shape promises: each path's totals stay below 2^64 (checked
    in floating point with room to spare for its rounding, then the wrapping sums are exact)."""
    d = seg_depth(steps, n_segs, path_begin, path_end)
    ids = np.asarray(steps, np.uint32) >> 1
    lens = np.asarray(seg_len, np.uint32).astype(np.uint64)
    assert int(d.max(initial=0)) < TWO32
    wl_f = lens.astype(np.float64) * d.astype(np.float64)
    assert float(wl_f.max(initial=0.0)) < 2.0 ** 63, "a segment's depth * length alone is near 2^64"
    wl = lens * d.astype(np.uint64)
    P = len(path_begin)
    length, weighted = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
    for p, (b, e) in enumerate(zip(path_begin, path_end)):
        s = ids[int(b):int(e)]
        if not len(s):
            continue
        est = float(wl_f[s].sum())  # (relative error far below 2^-40 for a few million addends)
        assert est < 2.0 ** 64 * (1 - 2.0 ** -30) or _exact_total(wl, s) < TWO64, "path %d: weighted total beyond 2^64" % p
        assert float(lens[s].astype(np.float64).sum()) < 2.0 ** 63
        length[p] = lens[s].sum(dtype=np.uint64)
        weighted[p] = wl[s].sum(dtype=np.uint64)
    return Twin(length, weighted, means(length.tolist(), weighted.tolist()), d)


def _exact_total(wl: np.ndarray, s: np.ndarray) -> int:
    """A total that the float estimate puts within 2^34 of 2^64: in Python ints, by distinct segment."""
    seg, cnt = np.unique(s, return_counts=True)
    return sum(int(wl[a]) * int(c) for a, c in zip(seg, cnt))
