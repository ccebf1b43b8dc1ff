"""An exact CPU model of path-pair overlap (slow_odgi/overlap.py:6-14), for the tests only, written apart from the kernels
of pollen_amd/csrc/overlap_device.hip and from the C oracle's bitset AND.

Path q touches path p when they are different paths and some ORIENTED handle (the step value itself: segment << 1 |
orientation) lies in both of their spans.  A span is [begin, end) of the step array as given: spans may overlap, nest,
repeat or be empty.  Two ways of asking, both exact:

- touch_rows: one row per query, O(N) per row -- the query's handles are marked, the marks gathered over the whole step
  array, and a prefix sum answers every span at once.  Meant for sampled rows of large graphs.
- touch_sparse: a self-join of the distinct (handle, path) pairs grouped by handle, O(sum of k^2) over the handles' path
  counts k.  Meant for whole matrices of sparse graphs.
"""
from __future__ import annotations

import numpy as np

# Above this many handles the mark array (one byte a handle) gives way to a sorted lookup of the query's handles.
MARK_MAX = 1 << 26


def _spans(begin, end):
    b = np.asarray(begin, dtype=np.int64)
    e = np.asarray(end, dtype=np.int64)
    assert b.shape == e.shape and (b <= e).all()
    return b, e


def touch_rows(steps, begin, end, n_segs: int, queries) -> np.ndarray:
    """uint8[len(queries), P]: row k says which paths touch path queries[k]."""
    steps = np.asarray(steps, dtype=np.uint32)
    b, e = _spans(begin, end)
    q = np.asarray(queries, dtype=np.int64)
    P = len(b)
    assert len(steps) == 0 or int(steps.max()) >> 1 < n_segs, "a step names a segment past n_segs"
    out = np.zeros((len(q), P), dtype=np.uint8)
    mark = np.zeros(2 * n_segs, dtype=np.uint8) if 2 * n_segs <= MARK_MAX else None
    cs = np.zeros(len(steps) + 1, dtype=np.int64)
    for k, ip in enumerate(q):
        assert 0 <= ip < P
        mine = steps[b[ip]:e[ip]]
        if mark is not None:
            mark[mine] = 1
            hit = mark[steps]
            mark[mine] = 0
        else:
            u = np.unique(mine)
            hit = (u[np.minimum(np.searchsorted(u, steps), max(len(u) - 1, 0))] == steps) if len(u) else np.zeros(len(steps), bool)
        np.cumsum(hit, out=cs[1:])
        row = (cs[e] - cs[b]) > 0
        row[ip] = False  # overlap.py:10-11: never a path with itself
        out[k] = row
    return out


def handle_path_pairs(steps, begin, end):
    """The distinct (handle, path) pairs, sorted by handle then path."""
    steps = np.asarray(steps, dtype=np.uint32)
    b, e = _spans(begin, end)
    n = e - b
    pid = np.repeat(np.arange(len(b), dtype=np.int64), n)
    idx = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n) + np.repeat(b, n)
    key = (steps[idx].astype(np.int64) << 32) | pid
    key = np.unique(key)
    return (key >> 32).astype(np.int64), (key & 0xFFFFFFFF).astype(np.int64)


def touch_sparse(steps, begin, end, n_segs: int, queries) -> np.ndarray:
    """The same matrix as touch_rows, from the handles that two or more paths share."""
    b, _ = _spans(begin, end)
    P = len(b)
    q = np.asarray(queries, dtype=np.int64)
    h, p = handle_path_pairs(steps, begin, end)
    assert len(h) == 0 or int(h.max()) >> 1 < n_segs, "a step names a segment past n_segs"
    _, start, k = np.unique(h, return_index=True, return_counts=True)
    many = k > 1
    start, k = start[many], k[many]
    kk = k * k
    total = int(kk.sum())
    t = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(kk) - kk, kk)
    ks, ss = np.repeat(k, kk), np.repeat(start, kk)
    a, c = p[ss + t // ks], p[ss + t % ks]
    # rows for the queries only: a path -> the query rows that ask for it
    order = np.argsort(q, kind="stable")
    qs = q[order]
    out = np.zeros((len(q), P), dtype=np.uint8)
    lo, hi = np.searchsorted(qs, a, "left"), np.searchsorted(qs, a, "right")
    n = hi - lo
    rows = order[np.repeat(lo, n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)]
    out[rows, np.repeat(c, n)] = 1
    out[np.arange(len(q)), q] = 0  # overlap.py:10-11
    return out
