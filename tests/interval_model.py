"""The model of interval depth over many paths (flatgfa_intervals_depth and the two tables on it).

intervals_depth is the reference's loop, group by group: a group is a maximal run of equal path ids, and each group is one
call of the oracle's interval_depth (oracle/flatgfa_oracle.py, pinned to window_depth.rs:84-147 by tests/test_oracle.py and
tests/f2_pins.py).  closed_form is what the kernels implement: per interval, independent of every other interval but for M,
the largest end among the intervals before it in its group.  tests/test_interval_model.py holds the two together bytewise.

Test infrastructure only."""
import bisect

import numpy as np

from oracle import flatgfa_oracle as fo


def runs(path_ids):
    """[(i0, i1)] of the maximal runs of equal ids."""
    ids = np.asarray(path_ids, dtype=np.int64)
    if not len(ids):
        return []
    cuts = np.flatnonzero(np.diff(ids)) + 1
    edges = np.concatenate([[0], cuts, [len(ids)]])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def intervals_depth(pools, path_ids, starts, ends) -> np.ndarray:
    st = np.asarray(starts, dtype=np.uint64)
    en = np.asarray(ends, dtype=np.uint64)
    out = np.zeros(len(st), np.float64)
    for a, b in runs(path_ids):
        out[a:b] = fo.interval_depth(pools, int(path_ids[a]), st[a:b], en[a:b])
    return out


def path_layout(pools, depth, pid):
    """(end positions r1 of the path's steps, their lengths, their segments' depths) as Python ints."""
    p = pools.paths[pid]
    segs = pools.steps[int(p["steps_start"]):int(p["steps_end"])].astype(np.int64) >> 1
    lens = [int(x) for x in pools.seg_lens()[segs]]
    r1, pos = [], 0
    for n in lens:
        pos += n
        r1.append(pos)
    return r1, lens, [int(depth[s]) for s in segs]


def closed_form(pools, path_ids, starts, ends, depth=None) -> np.ndarray:
    """out[i] = the sum, in increasing j from +0.0, over the steps j of the path with min(end, r1_j) > max(start, r0_j)
    and (i first in its group or r1_j >= M) of ((f64)(d_j * len_j) * ((f64)(o1 - o0) / (f64)len_j)) / (f64)(end - start):
    the steps from the first with r1_j >= max(start + 1, M) on, as long as r0_j < end."""
    depth = fo.seg_depth(pools) if depth is None else depth
    out = np.zeros(len(starts), np.float64)
    layouts = {}
    for a, b in runs(path_ids):
        pid = int(path_ids[a])
        if pid not in layouts:
            layouts[pid] = path_layout(pools, depth, pid)
        r1, lens, d = layouts[pid]
        m = 0
        for i in range(a, b):
            ws, we = int(starts[i]), int(ends[i])
            total = 0.0
            if we > ws:
                j = bisect.bisect_left(r1, max(ws + 1, m))
                while j < len(r1) and r1[j] - lens[j] < we:
                    r0 = r1[j] - lens[j]
                    o0, o1 = max(ws, r0), min(we, r1[j])
                    if o1 > o0:
                        total += (float(d[j] * lens[j]) * (float(o1 - o0) / float(lens[j]))) / float(we - ws)
                    j += 1
            out[i] = total
            m = max(m, we)
    return out


def windows(length: int, window: int):
    """make_windows, window_depth.rs:41-51"""
    rows, pos = [], 0
    while pos < length:
        e = min(pos + window, length)
        rows.append((pos, e))
        pos = e
    return rows


def window_depth_paths_table(pools, window: int, path_ids=None) -> bytes:
    """`fgfa window-depth P SIZE` of every listed path (default: all), one behind another."""
    ids = range(len(pools.paths)) if path_ids is None else path_ids
    return b"".join(fo.window_depth_table(pools, pools.path_name(int(p)), window) for p in ids)


def bed_depth_paths_table(pools, bed: bytes) -> bytes:
    """`fgfa depth -b`, every entry on the path it names: each run of one name is a group."""
    rows = fo.parse_bed(bed)
    ids = []
    for nm, _, _ in rows:
        pid = fo.find_path(pools, nm)
        if pid is None:
            raise fo.ParseError("path not found in graph")
        ids.append(pid)
    return fo._emit_intervals(rows, intervals_depth(pools, ids, [r[1] for r in rows], [r[2] for r in rows]))
