"""A plain-Python, sequential restatement of the reference's extract (flatgfa/src/ops/extract.rs, `fgfa extract`,
cli/cmds.rs:174-215), position (ops/position.rs, cli/cmds.rs:105-152) and the normalized printer (print.rs:127-142) over the
pools of oracle/flatgfa_oracle.py.  Test infrastructure only.

`variant` names one deliberate departure from a rule; tests/test_extract_shapes.py uses them to show that a shape really
exercises the rule it is aimed at (the answer changes when the rule does)."""
import numpy as np

from oracle import flatgfa_oracle as fo

VARIANTS = {
    "fifo",            # the frontier is popped from the front            (extract.rs:166 pops from the back)
    "from_only",       # a link is followed from `from` to `to` only      (flatgfa.rs:137-145 follows both ways)
    "last_name",       # find_seg takes the last segment of that name     (flatgfa.rs:380-384: the first)
    "fill_leading",    # the gap before the first member step is filled   (extract.rs:69, ignore_path)
    "fill_trailing",   # a gap still open at the path's end is filled     (extract.rs:71-97 fills on re-entry only)
    "gap_length",      # the bound is on the gap's length                 (extract.rs:68, 96: never reset, so a position)
    "lt",              # re-entry strictly before D                       (extract.rs:76: <=)
    "frozen_path",     # membership as it was when the path began         (extract.rs:72 reads the live map)
    "frozen_sweep",    # membership as it was when the sweep began
    "one_sweep",       # one sweep whatever num_iterations says           (extract.rs:181)
}


def find_seg(p: fo.Pools, name: int, variant=None):
    """flatgfa.rs:380-384: the first segment with that name, or None."""
    hits = [i for i, s in enumerate(p.segs) if int(s["name"]) == name]
    if not hits:
        return None
    return hits[-1] if variant == "last_name" else hits[0]


def _seg_len(p, seg):
    return int(p.segs[seg]["seq_end"]) - int(p.segs[seg]["seq_start"])


def neighbourhood(p: fo.Pools, origin: int, dist: int, variant=None):
    """extract.rs:159-178.  The old segment ids in the order they are included (= new id order)."""
    order, seg_map = [origin], {origin: 0}
    frontier, next_frontier = [origin], []
    links = [(int(l["from_"]) >> 1, int(l["to"]) >> 1) for l in p.links]
    for _ in range(dist):
        if not frontier:  # (what every further level of the reference finds: nothing to pop)
            break
        while frontier:
            seg = frontier.pop(0) if variant == "fifo" else frontier.pop()  # :166
            for f, t in links:  # :167 -- all links, in link order
                # Link::incident_seg, flatgfa.rs:137-145
                if f == seg:
                    other = t
                elif t == seg and variant != "from_only":
                    other = f
                else:
                    continue
                if other not in seg_map:  # :170-173
                    seg_map[other] = len(order)
                    order.append(other)
                    next_frontier.append(other)
        frontier, next_frontier = next_frontier, frontier  # :177
    return order, seg_map


def merge_subpaths(p: fo.Pools, path, max_dist: int, order, seg_map, variant=None, frozen=None):
    """extract.rs:65-98 for one path."""
    steps = [int(h) for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]]
    member = frozen if frozen is not None else (dict(seg_map) if variant == "frozen_path" else seg_map)
    cur_start, length, ignore = 0, 0, variant != "fill_leading"  # :67-69
    gap_len = 0

    def fill(a, b):
        for h in steps[a:b]:  # :82-86
            if (h >> 1) not in seg_map:
                seg_map[h >> 1] = len(order)
                order.append(h >> 1)

    for idx, h in enumerate(steps):  # :71
        in_neighb = (h >> 1) in member  # :72
        if cur_start is not None and in_neighb:  # :74
            bound = gap_len if variant == "gap_length" else length
            if not ignore and (bound < max_dist if variant == "lt" else bound <= max_dist):  # :76
                fill(cur_start, idx)
            cur_start, ignore = None, False  # :88-89
        elif cur_start is None and not in_neighb:  # :90
            cur_start, gap_len = idx, 0  # :92
        length += _seg_len(p, h >> 1)  # :96 -- never reset: the base position of the next step
        gap_len += _seg_len(p, h >> 1)
    if variant == "fill_trailing" and cur_start is not None and not ignore:
        fill(cur_start, len(steps))


def extract(p: fo.Pools, origin: int, dist: int, max_dist: int = 300000, iters: int = 6, variant=None) -> fo.Pools:
    """SubgraphBuilder::extract (extract.rs:152-198) with add_header (:27-34): the new store's pools."""
    assert variant is None or variant in VARIANTS
    if not 0 <= origin < len(p.segs):
        raise IndexError("origin segment out of range")
    for h in p.steps:
        if (int(h) >> 1) >= len(p.segs):
            raise IndexError("a step names a segment that is not there")
    for l in p.links:
        if (int(l["from_"]) >> 1) >= len(p.segs) or (int(l["to"]) >> 1) >= len(p.segs):
            raise IndexError("a link names a segment that is not there")
    order, seg_map = neighbourhood(p, origin, dist, variant)
    for _ in range(1 if variant == "one_sweep" and iters else iters):  # :181-185
        frozen = dict(seg_map) if variant == "frozen_sweep" else None
        for path in p.paths:
            merge_subpaths(p, path, max_dist, order, seg_map, variant, frozen)

    # include_seg (:37-45) in inclusion order
    segs = np.zeros(len(order), fo.SEG_DT)
    seq, opt = bytearray(), bytearray()
    for k, old in enumerate(order):
        s = p.segs[old]
        a, b = len(seq), len(opt)
        seq += p.seq_data[int(s["seq_start"]):int(s["seq_end"])].tobytes()
        opt += p.optional_data[int(s["opt_start"]):int(s["opt_end"])].tobytes()
        segs[k] = (int(s["name"]), a, len(seq), b, len(opt))

    def tr(h):  # :137-140
        return (seg_map[h >> 1] << 1) | (h & 1)

    # links (:188-192, include_link :48-53)
    links, align = [], []
    for l in p.links:
        f, t = int(l["from_"]), int(l["to"])
        if (f >> 1) in seg_map and (t >> 1) in seg_map:
            a = len(align)
            align += [int(x) for x in p.alignment[int(l["ov_start"]):int(l["ov_end"])]]
            links.append((tr(f), tr(t), a, len(align)))
    # find_subpaths (:102-134, include_subpath :56-61)
    steps, paths, names = [], [], bytearray()

    def include_subpath(path, start_step, start_pos, end_pos):
        nm = p.name_data[int(path["name_start"]):int(path["name_end"])].tobytes() + b":%d-%d" % (start_pos, end_pos)
        a = len(names)
        names.extend(nm)
        paths.append((a, len(names), start_step, len(steps), 0, 0))  # (no overlaps: the empty span of an empty pool)

    for path in p.paths:
        cur, pos = None, 0
        for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]:
            h = int(h)
            in_neighb = (h >> 1) in seg_map
            if cur is not None and not in_neighb:  # :109-112
                include_subpath(path, cur[0], cur[1], pos)
                cur = None
            elif cur is None and in_neighb:  # :113-119
                cur = (len(steps), pos)
            if in_neighb:  # :122-124
                steps.append(tr(h))
            pos += _seg_len(p, h >> 1)  # :127
        if cur is not None:  # :131-133
            include_subpath(path, cur[0], cur[1], pos)
    pt = np.zeros(len(paths), fo.PATH_DT)
    for i, r in enumerate(paths):
        pt[i] = r
    lk = np.zeros(len(links), fo.LINK_DT)
    for i, r in enumerate(links):
        lk[i] = r
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy()  # noqa: E731
    return fo.Pools(header=p.header.copy(), segs=segs, paths=pt, links=lk, steps=np.array(steps, np.uint32), seq_data=u8(seq),
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.array(align, np.uint32), name_data=u8(names),
                    optional_data=u8(opt), line_order=np.zeros(0, np.uint8))


def extract_by_name(p: fo.Pools, name: int, dist: int, max_dist: int = 300000, iters: int = 6, variant=None):
    """cmds.rs:200-215: None where the reference says "segment not found"."""
    origin = find_seg(p, name, variant)
    return None if origin is None else extract(p, origin, dist, max_dist, iters, variant)


_OPS = "MNDI"  # print.rs:13-22 (Insertion prints D, Deletion prints I)


def _align(p, a, b):
    ops = p.alignment[a:b]
    if len(ops) > 4096:  # (megabase spans: every distinct op is formatted once)
        u, inv = np.unique(ops, return_inverse=True)
        words = [b"%d%s" % (int(o) >> 8, _OPS[int(o) & 0xFF].encode()) for o in u]
        return b"".join(map(words.__getitem__, inv.tolist()))
    return b"0M" if len(ops) == 0 else b"".join(b"%d%s" % (int(o) >> 8, _OPS[int(o) & 0xFF].encode()) for o in ops)


def text(p: fo.Pools) -> bytes:
    """print.rs:127-142: header, segments, paths, links (a store with an empty line_order)."""
    assert len(p.line_order) == 0
    out = []
    if len(p.header):
        out.append(b"H\t" + p.header.tobytes())
    name = lambda h: b"%d%s" % (int(p.segs[int(h) >> 1]["name"]), b"-" if int(h) & 1 else b"+")  # noqa: E731
    for s in p.segs:
        ln = b"S\t%d\t" % int(s["name"]) + p.seq_data[int(s["seq_start"]):int(s["seq_end"])].tobytes()
        if int(s["opt_end"]) > int(s["opt_start"]):
            ln += b"\t" + p.optional_data[int(s["opt_start"]):int(s["opt_end"])].tobytes()
        out.append(ln)
    for path in p.paths:
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])]
        ov = p.overlaps[int(path["ov_start"]):int(path["ov_end"])]
        out.append(b"P\t" + p.name_data[int(path["name_start"]):int(path["name_end"])].tobytes() + b"\t" + b",".join(name(h) for h in st) +
                   b"\t" + (b"*" if len(ov) == 0 else b",".join(_align(p, int(o["start"]), int(o["end"])) for o in ov)))
    for l in p.links:
        f, t = int(l["from_"]), int(l["to"])
        out.append(b"L\t%d\t%s\t%d\t%s\t" % (int(p.segs[f >> 1]["name"]), b"-" if f & 1 else b"+", int(p.segs[t >> 1]["name"]),
                                               b"-" if t & 1 else b"+") + _align(p, int(l["ov_start"]), int(l["ov_end"])))
    return b"".join(ln + b"\n" for ln in out)


def position(p: fo.Pools, path_id: int, offset: int):
    """ops/position.rs:3-21: (handle, offset into the step), or None."""
    path = p.paths[path_id]
    cur = 0
    for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]:
        end = cur + _seg_len(p, int(h) >> 1)
        if offset < end:
            return int(h), offset - cur
        cur = end
    return None


class PositionError(Exception):
    """An Err of cmds::position (its message), or its assert."""


def position_table(p: fo.Pools, triple: bytes) -> bytes:
    """cmds.rs:114-152: what `fgfa position -p triple` prints."""
    parts = triple.split(b",")
    if len(parts) != 3:
        raise PositionError("position must be path_name,offset,orientation")
    t = parts[1][1:] if parts[1][:1] == b"+" else parts[1]  # usize::from_str
    if not t or not all(48 <= c <= 57 for c in t) or int(t) >= 1 << 64:
        raise PositionError("offset must be a number")
    offset = int(t)
    if parts[2] not in (b"+", b"-"):
        raise PositionError("orientation must be + or -")
    pid = fo.find_path(p, parts[0])
    if pid is None:
        raise PositionError("path not found")
    if parts[2] != b"+":
        raise PositionError("only + is implemented so far")
    hit = position(p, pid, offset)
    if hit is None:
        return b""
    h, off = hit
    return b"#source.path.pos\ttarget.graph.pos\n%s,%d,+\t%d,%d,%s\n" % (parts[0], offset, int(p.segs[h >> 1]["name"]), off,
                                                                         b"-" if h & 1 else b"+")


def extract_fast(p: fo.Pools, origin: int, dist: int, max_dist: int = 300000, iters: int = 6) -> fo.Pools:
    """The same pools with numpy passes over the links and the steps (one link pass per level; the merge walks each path's
    prefix of steps that start at or before max_dist), for graphs of millions of steps.  Pinned to extract() by
    tests/test_extract_model.py.  Path spans must tile the steps pool in path order."""
    S, NONE = len(p.segs), np.int64(-1)
    new = np.full(S, NONE)
    new[origin] = 0
    order = [origin]
    f, t = p.links["from_"].astype(np.int64) >> 1, p.links["to"].astype(np.int64) >> 1
    idx = np.arange(len(f), dtype=np.int64)
    front = np.array([origin], np.int64)
    for _ in range(dist):
        if not len(front):
            break
        rank = np.full(S, NONE)
        rank[front] = np.arange(len(front) - 1, -1, -1)  # popped from the back
        key = np.full(S, np.iinfo(np.int64).max)
        for a, b in ((f, t), (t, f)):
            m = (rank[a] >= 0) & (new[b] < 0) & (a != b)
            np.minimum.at(key, b[m], (rank[a[m]] << 32) | idx[m])
        cand = np.flatnonzero(key != np.iinfo(np.int64).max)
        front = cand[np.argsort(key[cand], kind="stable")]
        new[front] = len(order) + np.arange(len(front))
        order += [int(x) for x in front]
    lens = (p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"].astype(np.int64))
    seg = p.steps.astype(np.int64) >> 1
    b, e = p.paths["steps_start"].astype(np.int64), p.paths["steps_end"].astype(np.int64)
    assert len(b) == 0 or (b[0] == 0 and np.array_equal(b[1:], e[:-1]) and e[-1] == len(seg))
    cum = np.concatenate([[0], np.cumsum(lens[seg])])
    pid = np.repeat(np.arange(len(b)), e - b)
    pos = cum[:-1] - cum[b][pid]
    for _ in range(iters):
        before = len(order)
        for k in range(len(b)):
            n = int(np.searchsorted(pos[b[k]:e[k]], max_dist, side="right"))
            st = seg[b[k]:b[k] + n]
            if not (new[st] >= 0).any():
                continue
            cur, ignore = 0, True
            for i in range(n):
                inn = new[st[i]] >= 0
                if cur is not None and inn:
                    if not ignore:
                        for s in st[cur:i]:
                            if new[s] < 0:
                                new[s] = len(order)
                                order.append(int(s))
                    cur, ignore = None, False
                elif cur is None and not inn:
                    cur = i
        if len(order) == before:
            break
    order = np.array(order, np.int64)
    segs = np.zeros(len(order), fo.SEG_DT)
    sl = lens[order]
    ol = p.segs["opt_end"].astype(np.int64)[order] - p.segs["opt_start"].astype(np.int64)[order]
    so, oo = np.concatenate([[0], np.cumsum(sl)]), np.concatenate([[0], np.cumsum(ol)])
    segs["name"], segs["seq_start"], segs["seq_end"], segs["opt_start"], segs["opt_end"] = p.segs["name"][order], so[:-1], so[1:], oo[:-1], oo[1:]

    def gather(pool, starts, ln, offs):
        src = np.repeat(starts - offs[:-1], ln) + np.arange(int(offs[-1]), dtype=np.int64)
        return pool[src] if len(src) else pool[:0].copy()

    seq = gather(p.seq_data, p.segs["seq_start"].astype(np.int64)[order], sl, so)
    opt = gather(p.optional_data, p.segs["opt_start"].astype(np.int64)[order], ol, oo)
    keep = (new[f] >= 0) & (new[t] >= 0)
    lk = np.zeros(int(keep.sum()), fo.LINK_DT)
    al = (p.links["ov_end"].astype(np.int64) - p.links["ov_start"].astype(np.int64))[keep]
    ao = np.concatenate([[0], np.cumsum(al)])
    lk["from_"] = (new[f[keep]] << 1) | (p.links["from_"][keep] & 1)
    lk["to"] = (new[t[keep]] << 1) | (p.links["to"][keep] & 1)
    lk["ov_start"], lk["ov_end"] = ao[:-1], ao[1:]
    align = gather(p.alignment, p.links["ov_start"].astype(np.int64)[keep], al, ao)
    mem = new[seg] >= 0
    head = np.zeros(len(seg), bool)
    head[b[b < e]] = True
    prev = np.concatenate([[False], mem[:-1]])
    start = mem & (head | ~prev)
    nxt_mem = np.concatenate([mem[1:], [False]])
    nxt_head = np.concatenate([head[1:], [True]])
    end = mem & (nxt_head | ~nxt_mem)
    newidx = np.cumsum(mem) - mem
    si, ei = np.flatnonzero(start), np.flatnonzero(end)
    pt = np.zeros(len(si), fo.PATH_DT)
    names = bytearray()
    for k in range(len(si)):
        path = p.paths[pid[si[k]]]
        a = len(names)
        names += p.name_data[int(path["name_start"]):int(path["name_end"])].tobytes() + b":%d-%d" % (pos[si[k]], pos[ei[k]] + lens[seg[ei[k]]])
        pt[k] = (a, len(names), newidx[si[k]], newidx[ei[k]] + 1, 0, 0)
    steps = ((new[seg[mem]] << 1) | (p.steps[mem] & 1)).astype(np.uint32)
    return fo.Pools(header=p.header.copy(), segs=segs, paths=pt, links=lk, steps=steps, seq_data=seq.astype(np.uint8),
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=align.astype(np.uint32), name_data=np.frombuffer(bytes(names), np.uint8).copy(),
                    optional_data=opt.astype(np.uint8), line_order=np.zeros(0, np.uint8))
