"""The geometry of tests/test_gpu_inject_geometry.py: graph images as plain arrays (segment lengths, steps, path spans) with
BED lines on them, at the sizes where a kernel of inject_device.hip can go wrong, and a vectorized numpy form of the one-pass
model that answers them (the slow forms of tests/inject_model.py take minutes at 3 * 2^20 steps).  tests/test_inject_shapes.py
pins the fast form to the slow one on the CPU.  Test infrastructure only."""
from dataclasses import dataclass

import numpy as np

from oracle import flatgfa_oracle as fo

TILE = 256          # expand_kernels.hpp kTile: source elements per tile
OUT_TILE = 2048     # kOutTile: output items per k_expand / k_copy_lines workgroup
SCAN_TILE = 1024    # inject_device.hip kScanTile: elements per workgroup of the tiled scans
LINEAR = 16         # kLinear: cut rows up to this long are sorted by one lane


@dataclass
class Image:
    seg_len: np.ndarray      # int64[S]
    steps: np.ndarray        # int64[N]: segment << 1 | backward
    path_begin: np.ndarray   # int64[P]
    path_end: np.ndarray
    line_path: np.ndarray    # int64[n]
    lo: np.ndarray
    hi: np.ndarray


@dataclass
class Answer:
    seg_len: np.ndarray
    seg_first: np.ndarray
    steps: np.ndarray
    path_begin: np.ndarray
    path_end: np.ndarray


def image(seg_len, paths, lines) -> Image:
    """paths: arrays of handles, laid one behind another; lines: (path, lo, hi)."""
    n = np.array([len(h) for h in paths], dtype=np.int64)
    end = np.cumsum(n)
    ln = np.array(lines, dtype=np.int64).reshape(-1, 3)
    return Image(np.asarray(seg_len, dtype=np.int64), np.concatenate([np.asarray(h, dtype=np.int64) for h in paths] + [np.zeros(0, np.int64)]),
                 end - n, end, ln[:, 0].copy(), ln[:, 1].copy(), ln[:, 2].copy())


def fast(im: Image) -> Answer:
    """The one-pass model by searchsorted and repeat; a Python loop over the paths that lines name only."""
    S, n = len(im.seg_len), len(im.line_path)
    seg = im.steps >> 1
    bw = im.steps & 1
    if len(seg) and seg.max() >= S:
        raise IndexError("a step names a segment that is not there")
    if n and (im.line_path.max() >= len(im.path_begin) or im.line_path.min() < 0):
        raise IndexError("a line names a path that is not there")
    pre = np.concatenate([[0], np.cumsum(im.seg_len[seg])]).astype(np.int64)
    # locate: per line end, the step that holds it (the path's step count when none) and the cut
    at = np.zeros((n, 2), np.int64)      # step index within the path
    cseg = np.full((n, 2), -1, np.int64)
    cpos = np.zeros((n, 2), np.int64)
    j0 = np.zeros(n, np.int64)           # the first step with walk >= low
    for p in np.unique(im.line_path):
        b, e = int(im.path_begin[p]), int(im.path_end[p])
        walk = pre[b:e + 1] - pre[b]
        rows = np.flatnonzero(im.line_path == p)
        j0[rows] = np.searchsorted(walk[:e - b], im.lo[rows], side="left")
        for side, x in ((0, im.lo[rows]), (1, im.hi[rows])):
            i = np.searchsorted(walk[1:], x, side="right")
            at[rows, side] = i
            ok = i < e - b
            ic = np.minimum(i, max(e - b - 1, 0))
            cut = ok & (walk[ic] < x) if e > b else np.zeros(len(rows), bool)
            h = im.steps[b + ic] if e > b else np.zeros(len(rows), np.int64)
            o = x - walk[ic]
            cseg[rows, side] = np.where(cut, h >> 1, -1)
            cpos[rows, side] = np.where(cut, np.where(h & 1, im.seg_len[h >> 1] - o, o), 0)
    # the cut table
    have = cseg >= 0
    keys = np.unique((cseg[have] << 32) | cpos[have])
    k = np.bincount(keys >> 32, minlength=S).astype(np.int64) if len(keys) else np.zeros(S, np.int64)
    cut_row = np.concatenate([[0], np.cumsum(k)])
    cuts = keys & 0xFFFFFFFF
    first = np.concatenate([[0], np.cumsum(k + 1)])
    # new segments
    old = np.repeat(np.arange(S), k + 1)
    piece = np.arange(int(first[-1])) - first[old]
    cpad = np.concatenate([cuts, [0]])
    lo_edge = np.where(piece == 0, 0, cpad[np.maximum(cut_row[old] + piece - 1, 0)])
    hi_edge = np.where(piece == k[old], im.seg_len[old], cpad[np.minimum(cut_row[old] + piece, len(cuts))])
    # old paths, in path order (any spans)
    cnt = im.path_end - im.path_begin
    idx = (np.repeat(im.path_begin - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))).astype(np.int64)
    kk = k[seg[idx]] + 1
    offs = np.concatenate([[0], np.cumsum(kk)])
    rep = np.repeat(np.arange(len(idx)), kk)
    pc = np.arange(int(offs[-1])) - offs[rep]
    base, kr, b2 = first[seg[idx]][rep], kk[rep], bw[idx][rep]
    steps = np.where(b2 == 0, (base + pc) << 1, ((base + kr - 1 - pc) << 1) | 1)
    pstart = np.concatenate([[0], np.cumsum(cnt)])
    new_b, new_e = offs[pstart[:-1]], offs[pstart[1:]]
    # new paths
    rel = np.zeros((n, 2), np.int64)
    for side in (0, 1):
        i = np.where((side == 0) & ~have[:, 0], j0, at[:, side])
        pos_in_path = pstart[im.line_path] + i        # index into idx / offs
        w = np.zeros(n, np.int64)
        c = have[:, side]
        if c.any():
            sg, ps = cseg[c, side], cpos[c, side]
            r = np.searchsorted(keys, (sg << 32) | ps) - cut_row[sg]
            back = bw[idx[pos_in_path[c]]]
            w[c] = np.where(back == 1, k[sg] - r, r + 1)
        rel[:, side] = offs[pos_in_path] - offs[pstart[im.line_path]] + w
    length = np.maximum(rel[:, 1] - rel[:, 0], 0)
    src0 = new_b[im.line_path] + rel[:, 0] if n else np.zeros(0, np.int64)
    lend = np.cumsum(length)
    lbeg = lend - length
    src = (np.repeat(src0 - lbeg, length) + np.arange(int(length.sum()))).astype(np.int64)
    N_old = int(offs[-1])
    return Answer(hi_edge - lo_edge, first, np.concatenate([steps, steps[src]]).astype(np.int64),
                  np.concatenate([new_b, N_old + lbeg]).astype(np.int64), np.concatenate([new_e, N_old + lend]).astype(np.int64))


# ---- the slow model's answer on the same image ----
def pools_of(im: Image) -> fo.Pools:
    """Pools with sequence spans of the given lengths (seq_data itself is not needed by the model) and paths p0, p1, ..."""
    S, P = len(im.seg_len), len(im.path_begin)
    sg = np.zeros(S, fo.SEG_DT)
    end = np.cumsum(im.seg_len)
    sg["name"], sg["seq_start"], sg["seq_end"] = np.arange(1, S + 1), end - im.seg_len, end
    names = [b"p%d" % i for i in range(P)]
    pt = np.zeros(P, fo.PATH_DT)
    at = 0
    for i, nm in enumerate(names):
        pt[i] = (at, at + len(nm), im.path_begin[i], im.path_end[i], 0, 0)
        at += len(nm)
    e8 = np.zeros(0, np.uint8)
    return fo.Pools(header=e8, segs=sg, paths=pt, links=np.zeros(0, fo.LINK_DT), steps=im.steps.astype(np.uint32), seq_data=e8,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(b"".join(names), np.uint8),
                    optional_data=e8, line_order=e8)


def slow(im: Image) -> Answer:
    import inject_model as m
    p = pools_of(im)
    lines = [(b"p%d" % int(q), int(a), int(b), b"n%d" % i) for i, (q, a, b) in enumerate(zip(im.line_path, im.lo, im.hi))]
    q = m.inject(p, lines)
    return Answer((q.segs["seq_end"].astype(np.int64) - q.segs["seq_start"]), m.seg_first(p, lines), q.steps.astype(np.int64),
                  q.paths["steps_start"].astype(np.int64), q.paths["steps_end"].astype(np.int64))


def same(a: Answer, b: Answer) -> bool:
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("seg_len", "seg_first", "steps", "path_begin", "path_end"))


# ---- shapes ----
def random_image(rng, n_segs, n_paths, max_steps, n_lines, max_len=6, zero=0.1) -> Image:
    seg_len = rng.integers(1, max_len + 1, n_segs)
    seg_len[rng.random(n_segs) < zero] = 0
    counts = [int(rng.integers(1, max_steps + 1)) for _ in range(n_paths)]
    paths = [(rng.integers(0, n_segs, c) << 1) | rng.integers(0, 2, c) for c in counts]
    lens = [int(seg_len[h >> 1].sum()) for h in paths]
    lines = []
    for _ in range(n_lines):
        p = int(rng.integers(0, n_paths))
        a, b = sorted(int(x) for x in rng.integers(0, lens[p] + 3, 2))
        if rng.random() < 0.1:
            a, b = b, a
        lines.append((p, a, b))
    return image(seg_len, paths, lines)


def line_counts(n_lines, seed=3) -> Image:
    """n lines on a graph of 40 segments and 3 short paths: the lane-per-line kernels' grids, the row sort (every segment is cut
    by thousands of lines once n is large), the scans over lines."""
    rng = np.random.default_rng(seed)
    seg_len = rng.integers(2, 40, 40)
    paths = [(rng.integers(0, 40, 30) << 1) | rng.integers(0, 2, 30) for _ in range(3)]
    lens = np.array([int(seg_len[h >> 1].sum()) for h in paths])
    p = rng.integers(0, 3, n_lines)
    a = rng.integers(0, lens[p] + 2)
    b = np.minimum(a + rng.integers(0, 6, n_lines), lens[p] + 2)  # (short intervals: the new steps stay few)
    return image(seg_len, paths, np.stack([p, a, b], axis=1))


def seam_ends(k=2) -> Image:
    """Segments of 3 bases, one path over 256 k + 40 steps after a first path of 7: line ends on the seams at pool steps
    256 k - 1, 256 k, 256 k + 1, inside those steps, at each path's first and last step, on the first base, the last base and
    one past the end."""
    n2 = TILE * k + 40
    seg_len = np.full(64, 3)
    rng = np.random.default_rng(5)
    p0 = (rng.integers(0, 64, 7) << 1) | rng.integers(0, 2, 7)
    p1 = (rng.integers(0, 64, n2) << 1) | rng.integers(0, 2, n2)
    lines = []
    for pool_step in (TILE * k - 1, TILE * k, TILE * k + 1, 7, 7 + n2 - 1):
        i = pool_step - 7
        lines += [(1, 3 * i, 3 * i + 3), (1, 3 * i + 1, 3 * i + 5), (1, 3 * i - 2, 3 * i + 2), (1, 3 * i, 3 * i)]
    total = 3 * n2
    lines += [(1, 0, 1), (1, total - 1, total), (1, total - 1, total + 1), (1, total, total + 1), (1, 0, total), (0, 0, 21), (0, 20, 21), (0, 1, 22),
              (0, 6, 3)]
    lines = [(p, max(a, 0), b) for p, a, b in lines]
    return image(seg_len, [p0, p1], lines)


def cut_rows() -> Image:
    """Rows of 0, 1, 16, 17 and 4097 distinct cuts, a row that is one position many times over, cuts at 1 and len - 1, and a
    segment that is cut through a backward step only."""
    seg_len = np.array([50, 50, 50, 50, 5000, 50, 50, 50])
    fwd = np.arange(8) << 1
    path = np.concatenate([fwd, [(7 << 1) | 1]])  # p0: 0+ .. 7+ 7-
    start = np.concatenate([[0], np.cumsum(seg_len)])
    lines = [(0, int(start[1]) + 7, int(start[2]))]                                   # segment 1: one cut
    lines += [(0, int(start[2]) + i, int(start[2]) + i + 1) for i in range(1, 16, 2)]  # segment 2: 16 cuts (1..16)
    lines += [(0, int(start[3]) + i, int(start[4])) for i in range(1, 18)]             # segment 3: 17 cuts
    lines += [(0, int(start[4]) + i, int(start[5])) for i in range(1, 4098)]           # segment 4: 4097 cuts, in ...
    lines = lines[:40] + lines[:39:-1]                                                 # ... descending order
    lines += [(0, int(start[5]) + 9, int(start[6]))] * 300                             # segment 5: one position 300 times
    lines += [(0, int(start[6]) + 1, int(start[6]) + 49)]                              # segment 6: cuts at 1 and len - 1
    back = int(start[8])                                                               # 7- walks segment 7 a second time
    lines += [(0, back + 10, back + 50)]                                               # segment 7: position 40, through 7- only
    return image(seg_len, [path], lines)


def many_segments(S) -> Image:
    """S segments with a cut in the last one (and every 97th): seg_first crosses the tile edges."""
    seg_len = np.full(S, 4)
    path = np.arange(S) << 1
    lines = [(0, 4 * s + 1, 4 * s + 3) for s in list(range(0, S, 97)) + [S - 1]]
    return image(seg_len, [path], lines)


def expansion(total) -> Image:
    """A new steps pool of exactly `total` steps before the new paths: one path of steps that are cut into 1..5 pieces."""
    rng = np.random.default_rng(total)
    seg_len = np.full(200, 10)
    n = total // 3
    path = (rng.integers(0, 200, n) << 1) | rng.integers(0, 2, n)
    # cut the first 40 segments into 5 pieces; then pad with uncut steps of segment 199 to reach the total exactly
    lines = []
    first = {}
    for i, h in enumerate(path):
        first.setdefault(int(h) >> 1, i)
    for s in range(40):
        if s in first:
            i, h = first[s], int(path[first[s]])
            for o in (2, 4, 6, 8):
                lines.append((0, 10 * i + o, 10 * i + o))
    im = image(seg_len, [path], lines)
    have = len(fast(im).steps)
    assert have <= total
    path = np.concatenate([path, np.full(total - have, 199 << 1)])
    im = image(seg_len, [path], lines)
    return im


def whole_tiles_backward() -> Image:
    """One backward step of a segment with 4097 cuts: its pieces fill two output tiles and part of a third."""
    seg_len = np.array([3, 5000, 3])
    path = np.array([0 << 1, (1 << 1) | 1, 2 << 1])
    lines = [(0, 3 + i, 3 + i) for i in range(1, 4098)] + [(0, 4, 4100), (0, 0, 5006), (0, 2000, 2001)]
    return image(seg_len, [path], lines)


def overlapping_spans() -> Image:
    """Path spans that do not tile the pool (they overlap, leave a gap, and come out of order): the per-path route."""
    rng = np.random.default_rng(8)
    seg_len = rng.integers(1, 9, 30)
    steps = (rng.integers(0, 30, 700) << 1) | rng.integers(0, 2, 700)
    pb = np.array([300, 0, 250, 690, 5])
    pe = np.array([700, 280, 520, 690, 6])
    pre = np.concatenate([[0], np.cumsum(seg_len[steps >> 1])])
    lines = []
    for p in range(5):
        total = int(pre[pe[p]] - pre[pb[p]])
        for _ in range(12):
            a, b = sorted(int(x) for x in rng.integers(0, total + 2, 2))
            lines.append((p, a, b))
    ln = np.array(lines, dtype=np.int64)
    return Image(seg_len.astype(np.int64), steps.astype(np.int64), pb, pe, ln[:, 0].copy(), ln[:, 1].copy(), ln[:, 2].copy())


def long_and_short_lines(n_long=3 << 20) -> Image:
    """A path of 3 * 2^20 steps covered whole by one line, next to lines of 0, 1 and 3 steps, and a second path whose new path
    ends in the last step of the pool."""
    rng = np.random.default_rng(9)
    seg_len = np.full(1000, 2)
    p0 = (rng.integers(0, 1000, n_long) << 1) | rng.integers(0, 2, n_long)
    p1 = (rng.integers(0, 1000, 10) << 1) | rng.integers(0, 2, 10)
    lines = [(0, 4, 4), (0, 0, 2 * n_long), (0, 10, 12), (0, 20, 26), (1, 5, 5), (0, 2 * n_long - 3, 2 * n_long), (1, 3, 20)]
    return image(seg_len, [p0, p1], lines)


def many_lines_one_path(n=70001) -> Image:
    rng = np.random.default_rng(10)
    seg_len = rng.integers(1, 30, 500)
    p0 = (rng.integers(0, 500, 3000) << 1) | rng.integers(0, 2, 3000)
    p1 = (rng.integers(0, 500, 20) << 1) | rng.integers(0, 2, 20)
    total = int(seg_len[p0 >> 1].sum())
    a = rng.integers(0, total, n)
    b = a + rng.integers(0, 40, n)
    return image(seg_len, [p1, p0], np.stack([np.ones(n, np.int64), a, b], axis=1))


def unsorted_nested() -> Image:
    """Lines on paths in no order, nested and crossing intervals, low > high."""
    rng = np.random.default_rng(12)
    seg_len = rng.integers(1, 9, 60)
    paths = [(rng.integers(0, 60, 300) << 1) | rng.integers(0, 2, 300) for _ in range(4)]
    lines = [(3, 100, 900), (0, 5, 50), (3, 200, 800), (2, 0, 10), (3, 300, 301), (0, 0, 1000000), (1, 77, 70), (3, 100, 900), (2, 9, 9), (0, 49, 51)]
    return image(seg_len, paths, lines)


def limit(n_lines) -> Image:
    """A path of 2^20 steps and n lines that each cover it whole."""
    n = 1 << 20
    seg_len = np.full(16, 1)
    path = (np.arange(n) % 16) << 1
    return image(seg_len, [path], [(0, 0, n)] * n_lines)
