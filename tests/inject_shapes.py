"""The geometry of tests/test_gpu_inject_geometry.py and tests/test_gpu_inject_host_geometry.py: graph images as plain arrays
(segment lengths, steps, path spans; optionally seq starts, links and new names) with BED lines on them, at the sizes where a
kernel of inject_device.hip can go wrong, and a vectorized numpy form of the one-pass model that answers them (the slow forms
of tests/inject_model.py take minutes at 3 * 2^20 steps): `fast` for what the device entry returns, `fast_pools` for every pool
of the handle's result.  tests/test_inject_shapes.py pins both to the slow model on the CPU.  Test infrastructure only."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from oracle import flatgfa_oracle as fo

TILE = 256          # expand_kernels.hpp kTile: source elements per tile
OUT_TILE = 2048     # kOutTile: output items per k_expand / k_copy_lines workgroup
SCAN_TILE = 1024    # inject_device.hip kScanTile: elements per workgroup of the tiled scans
LINEAR = 16         # kLinear: cut rows up to this long are sorted by one lane
MAX_GRID = 2048     # kMaxGrid: workgroups of k_sort_long and k_sort_short, which stride over the rest


@dataclass
class Image:
    seg_len: np.ndarray      # int64[S]
    steps: np.ndarray        # int64[N]: segment << 1 | backward
    path_begin: np.ndarray   # int64[P]
    path_end: np.ndarray
    line_path: np.ndarray    # int64[n]
    lo: np.ndarray
    hi: np.ndarray
    seq_start: Optional[np.ndarray] = None   # int64[S]; None: one segment behind another
    links: Optional[np.ndarray] = None       # int64[L, 2]: (from, to) handles
    names: Optional[List[bytes]] = None      # the new paths' names; None: n0, n1, ...


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
    return _solve(im)[0]


def raw_rows(im: Image) -> np.ndarray:
    """int64[S]: the line ends that cut each segment, repeats counted -- the length of its row before the sort."""
    return _solve(im)[1]


def _solve(im: Image):
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
    raw = np.bincount(cseg[have], minlength=S).astype(np.int64) if have.any() else np.zeros(S, np.int64)
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
                  np.concatenate([new_b, N_old + lbeg]).astype(np.int64), np.concatenate([new_e, N_old + lend]).astype(np.int64)), raw


# ---- the image as pools, and the slow model's answer on it ----
BASES = np.frombuffer(b"ACGT", np.uint8)
COMPLEMENT = np.arange(256, dtype=np.uint8)
COMPLEMENT[list(b"ACGTacgt")] = list(b"TGCAtgca")


def new_names(im: Image) -> List[bytes]:
    return list(im.names) if im.names is not None else [b"n%d" % i for i in range(len(im.line_path))]


def lines_of(im: Image):
    """The lines as tests/inject_model.py and FlatGFA.inject's BED text take them: (path name, low, high, new name)."""
    return [(b"p%d" % int(q), int(a), int(b), nm) for q, a, b, nm in zip(im.line_path, im.lo, im.hi, new_names(im))]


def pools_of(im: Image) -> fo.Pools:
    """Pools with sequence spans of the given lengths (at im.seq_start; one behind another when there is none) over seq_data
    of fixed pseudo-random bases, the image's links, and paths p0, p1, ..."""
    S, P = len(im.seg_len), len(im.path_begin)
    sg = np.zeros(S, fo.SEG_DT)
    start = (np.cumsum(im.seg_len) - im.seg_len) if im.seq_start is None else np.asarray(im.seq_start, dtype=np.int64)
    sg["name"], sg["seq_start"], sg["seq_end"] = np.arange(1, S + 1), start, start + im.seg_len
    n_bases = int((start + im.seg_len).max()) if S else 0
    seq = BASES[((np.arange(n_bases, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(3)]
    names = [b"p%d" % i for i in range(P)]
    nlen = np.array([len(nm) for nm in names], dtype=np.int64)
    nend = np.cumsum(nlen)
    pt = np.zeros(P, fo.PATH_DT)
    pt["name_start"], pt["name_end"], pt["steps_start"], pt["steps_end"] = nend - nlen, nend, im.path_begin, im.path_end
    lk = np.zeros(0 if im.links is None else len(im.links), fo.LINK_DT)
    if len(lk):
        lk["from_"], lk["to"] = im.links[:, 0], im.links[:, 1]
    e8 = np.zeros(0, np.uint8)
    return fo.Pools(header=e8, segs=sg, paths=pt, links=lk, steps=im.steps.astype(np.uint32), seq_data=seq,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(b"".join(names), np.uint8),
                    optional_data=e8, line_order=e8)


def slow(im: Image) -> Answer:
    import inject_model as m
    p = pools_of(im)
    lines = lines_of(im)
    q = m.inject(p, lines)
    return Answer((q.segs["seq_end"].astype(np.int64) - q.segs["seq_start"]), m.seg_first(p, lines), q.steps.astype(np.int64),
                  q.paths["steps_start"].astype(np.int64), q.paths["steps_end"].astype(np.int64))


def fast_pools(im: Image, links: bool = False, p: Optional[fo.Pools] = None, answer: Optional[Answer] = None) -> fo.Pools:
    """Every pool of inject's result on `p` (pools_of(im) when not given; its segments, steps and path spans must be the
    image's), as inject_model.inject(p, lines_of(im), links) states them, from the vectorized answer (fast(im), or the one given)."""
    a = fast(im) if answer is None else answer
    if p is None:
        p = pools_of(im)
    S, P, n = len(im.seg_len), len(im.path_begin), len(im.line_path)
    first = a.seg_first
    k1 = np.diff(first)                                   # the pieces of each old segment
    S2 = int(first[-1])
    old = np.repeat(np.arange(S), k1)
    begin = np.cumsum(a.seg_len) - a.seg_len              # new segments laid one behind another ...
    within = begin - begin[first[:-1]][old]               # ... so this is where a piece starts in its old segment
    sg = np.zeros(S2, fo.SEG_DT)
    sg["name"] = np.arange(1, S2 + 1)
    sg["seq_start"] = p.segs["seq_start"].astype(np.int64)[old] + within
    sg["seq_end"] = sg["seq_start"].astype(np.int64) + a.seg_len
    # names: the old table, then the new names in line order
    fresh = new_names(im)
    old_names = {p.path_name(i) for i in range(P)}
    if len(set(fresh)) != n or old_names & set(fresh):
        raise ValueError("a new name is given twice or is a path of the graph: the model refuses these")
    flen = np.array([len(nm) for nm in fresh], dtype=np.int64)
    fend = len(p.name_data) + np.cumsum(flen)
    pt = np.zeros(P + n, fo.PATH_DT)
    pt["name_start"] = np.concatenate([p.paths["name_start"].astype(np.int64), fend - flen])
    pt["name_end"] = np.concatenate([p.paths["name_end"].astype(np.int64), fend])
    pt["steps_start"], pt["steps_end"] = a.path_begin, a.path_end
    lk = np.zeros(0, fo.LINK_DT)
    if links:
        ids = np.arange(S2, dtype=np.int64)
        intra = ids[ids - first[old] < k1[old] - 1]       # every piece but the last of its segment
        f, t = p.links["from_"].astype(np.int64), p.links["to"].astype(np.int64)
        fs, ts = f >> 1, t >> 1
        if len(f) and max(fs.max(), ts.max()) >= S:
            raise IndexError("a link names a segment that is not there")
        nf = np.where(f & 1 == 0, first[fs + 1] - 1, first[fs])
        nt = np.where(t & 1 == 0, first[ts], first[ts + 1] - 1)
        lk = np.zeros(len(intra) + len(f), fo.LINK_DT)
        lk["from_"] = np.concatenate([intra << 1, (nf << 1) | (f & 1)])
        lk["to"] = np.concatenate([(intra + 1) << 1, (nt << 1) | (t & 1)])
    e8 = np.zeros(0, np.uint8)
    return fo.Pools(header=p.header, segs=sg, paths=pt, links=lk, steps=a.steps.astype(np.uint32), seq_data=p.seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32),
                    name_data=np.concatenate([p.name_data, np.frombuffer(b"".join(fresh), np.uint8)]), optional_data=e8, line_order=e8)


def differing(a: fo.Pools, b: fo.Pools) -> List[str]:
    """The pools of fo.POOL_ORDER whose bytes differ: empty for the same graph (chop_model.same_pools, with names to report)."""
    return [n for n in fo.POOL_ORDER if getattr(a, n).tobytes() != getattr(b, n).tobytes()]


def spell(p: fo.Pools, path: int) -> bytes:
    """The bases a path spells: each step's sequence, reverse-complemented for a backward step."""
    out = []
    for h in p.steps[int(p.paths[path]["steps_start"]):int(p.paths[path]["steps_end"])]:
        s = p.segs[int(h) >> 1]
        b = p.seq_data[int(s["seq_start"]):int(s["seq_end"])]
        out.append(COMPLEMENT[b[::-1]].tobytes() if int(h) & 1 else b.tobytes())
    return b"".join(out)


def spell_pool(p: fo.Pools):
    """spell for the whole steps pool at once: (bases, off) with path i spelling bases[off[steps_start] : off[steps_end]]."""
    h = p.steps.astype(np.int64)
    st, en = p.segs["seq_start"].astype(np.int64)[h >> 1], p.segs["seq_end"].astype(np.int64)[h >> 1]
    off = np.concatenate([[0], np.cumsum(en - st)]).astype(np.int64)
    rep = np.repeat(np.arange(len(h), dtype=np.int32), en - st)
    k = np.arange(int(off[-1]), dtype=np.int64) - off[rep]
    back = (h & 1).astype(bool)[rep]
    b = p.seq_data[np.where(back, en[rep] - 1 - k, st[rep] + k)]
    return np.where(back, COMPLEMENT[b], b), off


def spelled(sp, p: fo.Pools, path: int) -> bytes:
    bases, off = sp
    return bases[off[int(p.paths[path]["steps_start"])]:off[int(p.paths[path]["steps_end"])]].tobytes()


def same(a: Answer, b: Answer) -> bool:
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("seg_len", "seg_first", "steps", "path_begin", "path_end"))

def check_spelling(im: Image, p: fo.Pools, q: fo.Pools, sp=None):
    """(a) every old path of q spells what it spelled in p; (b) new path l spells whole[lo:hi] of its path."""
    P = len(p.paths)
    sp = spell_pool(q) if sp is None else sp
    whole = [spell(p, i) for i in range(P)]
    for i in range(P):
        assert spelled(sp, q, i) == whole[i], i
    for l, (path, lo, hi) in enumerate(zip(im.line_path.tolist(), im.lo.tolist(), im.hi.tolist())):
        assert spelled(sp, q, P + l) == (whole[path][lo:hi] if lo <= hi else b""), l


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
    """S segments with a cut in the last one (and every 97th): seg_first crosses the tile edges.  Where S reaches the end of
    k_sort_short's first round (MAX_GRID * 256 segments a round), the last two segments of that round and the first of the next
    are 8 bases long and get a row of 5 cuts given in descending order, so that the second round is what sorts segment 524288."""
    seg_len = np.full(S, 4)
    rows = range(MAX_GRID * 256 - 2, min(S, MAX_GRID * 256 + 1))
    seg_len[list(rows)] = 8
    at = np.cumsum(seg_len) - seg_len
    path = np.arange(S) << 1
    lines = [(0, int(at[s]) + 1, int(at[s]) + 3) for s in list(range(0, S, 97)) + [S - 1]]
    lines += [(0, int(at[s]) + c, int(at[s]) + 8) for s in rows for c in (7, 6, 5, 4, 2)]
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


def long_rows(R) -> Image:
    """R segments of 40 bases on one path, each cut at 1 .. 17 by lines given in descending order of position (their other
    end is on the segment's last seam and cuts nothing); every 50th row has positions 5 and 9 three times more.  Every row is
    longer than LINEAR, so k_sort_long is given R rows: MAX_GRID of them a round."""
    path = np.arange(R) << 1
    lines = []
    for s in range(R):
        cuts = list(range(17, 0, -1))
        if s % 50 == 0:
            cuts = cuts[:9] + [9, 5, 9] + cuts[9:] + [5, 9, 5]
        lines += [(0, 40 * s + c, 40 * s + 40) for c in cuts]
    return image(np.full(R, 40), [path], lines)


ROW_LENGTHS = (31, 32, 33, 255, 256, 257, 511, 512, 513, 1025)


def row_lengths(rows=ROW_LENGTHS) -> Image:
    """One segment per entry of `rows` with a raw row of exactly that many keys, given in descending order: the bitonic
    network at, one under and one over a power of two, and at the 256-lane stride.  Every third row repeats a seventh of its keys."""
    S = len(rows)
    seg_len = np.full(S, 2000)
    lines = []
    for s, m in enumerate(rows):
        dup = m // 7 if s % 3 == 0 else 0
        cuts = list(range(m - dup, 0, -1))
        cuts += cuts[:dup]                       # (the first `dup` positions once more, behind the rest)
        assert len(cuts) == m and cuts[0] < 2000
        lines += [(0, 2000 * s + c, 2000 * s + 2000) for c in cuts]
    return image(seg_len, [np.arange(S) << 1], lines)


def pool_steps(N) -> Image:
    """Two tiling paths with N steps in all, over segments of 3 bases: lines that end inside the last step of the pool, on its
    last seam and one past its end (and the same on the first path), so that pre[N] and noff[N] are read."""
    rng = np.random.default_rng(N)
    n0 = 300
    p0 = (rng.integers(0, 64, n0) << 1) | rng.integers(0, 2, n0)
    p1 = (rng.integers(0, 64, N - n0) << 1) | rng.integers(0, 2, N - n0)
    lines = []
    for p, t in ((1, 3 * (N - n0)), (0, 3 * n0)):
        lines += [(p, t - 2, t - 1), (p, t - 5, t - 3), (p, t - 4, t), (p, t - 1, t + 1), (p, t, t + 1), (p, 0, t), (p, 1, t + 5), (p, t + 1, t + 2)]
    return image(np.full(64, 3), [p0, p1], lines)


def many_paths_non_tiling() -> Image:
    """4100 overlapping spans over a pool of 5000 steps (the per-path route), with lines on the first path, on the last of
    k_path_lens' and k_expand_paths' first round of 4096 workgroups, and on the first and the last of their second."""
    rng = np.random.default_rng(14)
    seg_len = rng.integers(1, 9, 300)
    steps = (rng.integers(0, 300, 5000) << 1) | rng.integers(0, 2, 5000)
    pb = rng.integers(0, 4980, 4100)
    pe = pb + rng.integers(1, 21, 4100)
    pre = np.concatenate([[0], np.cumsum(seg_len[steps >> 1])])
    lines = []
    for p in (0, 4095, 4096, 4099):
        total = int(pre[pe[p]] - pre[pb[p]])
        for _ in range(6):
            a, b = sorted(int(x) for x in rng.integers(0, total + 2, 2))
            lines.append((p, a, b))
    ln = np.array(lines, dtype=np.int64)
    return Image(seg_len.astype(np.int64), steps.astype(np.int64), pb, pe, ln[:, 0].copy(), ln[:, 1].copy(), ln[:, 2].copy())


# ---- links, seq spans and a ring, for the handle's route ----
def with_links(im: Image, L, seed=0) -> Image:
    """The image with L links: random ones over every segment and orientation, and in front of them (as far as L allows) both
    ends on cut segments in all four orientation pairs, self-loops s+ -> s+ and s+ -> s- on a cut segment, and one link thrice."""
    rng = np.random.default_rng(seed)
    S = len(im.seg_len)
    cut = np.flatnonzero(np.diff(fast(im).seg_first) > 1)
    a, b = (int(cut[0]), int(cut[-1])) if len(cut) else (0, S - 1)
    planted = [(a << 1, b << 1), (a << 1, (b << 1) | 1), ((a << 1) | 1, b << 1), ((a << 1) | 1, (b << 1) | 1), (a << 1, a << 1), (a << 1, (a << 1) | 1),
               (a << 1, b << 1), (a << 1, b << 1), ((b << 1) | 1, (b << 1) | 1)]
    rnd = np.stack([(rng.integers(0, S, L) << 1) | rng.integers(0, 2, L), (rng.integers(0, S, L) << 1) | rng.integers(0, 2, L)], axis=1)
    if len(cut) and L:  # (half of the random ones leave a cut segment, too)
        rnd[::2, 0] = (cut[rng.integers(0, len(cut), len(rnd[::2]))] << 1) | (rnd[::2, 0] & 1)
    lk = np.concatenate([np.array(planted, dtype=np.int64).reshape(-1, 2), rnd.astype(np.int64)])[:L]
    return Image(im.seg_len, im.steps, im.path_begin, im.path_end, im.line_path, im.lo, im.hi, im.seq_start, lk, im.names)


def scattered_spans(im: Image, seed=0) -> Image:
    """The image with seq spans that are not one behind another: anywhere in a seq_data no longer than the longest segment
    plus 37, so that they alias one another, run backwards through it and leave gaps (as flatten_shapes.f_alias_backwards)."""
    rng = np.random.default_rng(seed)
    room = int(im.seg_len.max()) + 37 if len(im.seg_len) else 0
    start = rng.integers(0, room - im.seg_len + 1)
    return Image(im.seg_len, im.steps, im.path_begin, im.path_end, im.line_path, im.lo, im.hi, start.astype(np.int64), im.links, im.names)


def ring(S=3000, n_lines=5000) -> Image:
    """S segments linked i+ -> (i + 1)+ into a ring; one path goes round it twice forwards, one goes round backwards; both are
    walks of the links, and so is every interval of them."""
    rng = np.random.default_rng(15)
    seg_len = rng.integers(1, 12, S)
    fwd = np.arange(S) << 1
    p0 = np.concatenate([fwd, fwd])
    p1 = fwd[::-1] | 1
    lens = np.array([2 * int(seg_len.sum()), int(seg_len.sum())])
    p = rng.integers(0, 2, n_lines)
    a = rng.integers(0, lens[p])
    b = np.minimum(a + rng.integers(0, 60, n_lines), lens[p] + 1)
    im = image(seg_len, [p0, p1], np.stack([p, a, b], axis=1))
    im.links = np.stack([fwd, np.roll(fwd, -1)], axis=1).astype(np.int64)
    return im
