"""A plain-Python restatement of the reference's chop (flatgfa/src/ops/chop.rs, with `fgfa chop`'s output store,
cli/main.rs:139-159) over the pools of oracle/flatgfa_oracle.py, and a vectorized numpy form of the same for graphs of tens
of millions of steps (pinned to the slow form by tests/test_chop_model.py).  Test infrastructure only."""
import os
import tempfile

import numpy as np

from oracle import flatgfa_oracle as fo

E8 = lambda n=0: np.zeros(n, np.uint8)  # noqa: E731


def _store(p, segs, paths, links, steps):
    # cli/main.rs:145-158: header, seq_data and name_data from the input; the rest from chop's store, whose overlaps,
    # alignment, optional_data and line_order stay empty (so the text comes out in normalized order, print.rs:128-150)
    return fo.Pools(header=p.header, segs=segs, paths=paths, links=links, steps=steps, seq_data=p.seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=p.name_data,
                    optional_data=E8(), line_order=E8())


def chop(p: fo.Pools, c: int, links: bool = False) -> fo.Pools:
    """chop.rs, rule by rule.  ValueError for c == 0 (chop.rs:43-50 loops forever); IndexError where a step or a link names a
    segment that is not there (chop.rs:74, :112, :121 index seg_map)."""
    if c <= 0:
        raise ValueError("max_size 0: the reference loops forever")
    segs, seg_map, new_links = [], [], []
    # chop.rs:25-66
    for s in p.segs:
        start, end = int(s["seq_start"]), int(s["seq_end"])
        if end - start <= c:  # :27-35 -- kept whole, including length 0
            segs.append((len(segs) + 1, start, end))
            seg_map.append((len(segs) - 1, len(segs)))
        else:
            first, off = len(segs), start
            while off < end - c:  # :43-50 -- pieces of c
                segs.append((len(segs) + 1, off, off + c))
                off += c
            segs.append((len(segs) + 1, off, end))  # :52-57 -- the remainder
            seg_map.append((first, len(segs)))
            if links:  # :62-64, link_forward :14-22
                new_links += [((i << 1), ((i + 1) << 1)) for i in range(first, len(segs) - 1)]
    # chop.rs:68-104
    steps, paths = [], []
    for path in p.paths:
        path_start = len(steps)
        for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]:
            a, b = seg_map[int(h) >> 1]
            if int(h) & 1 == 0:  # :80-85 forward
                steps += [i << 1 for i in range(a, b)]
            else:  # :86-95 backward: the same ids, reversed
                steps += [(i << 1) | 1 for i in reversed(range(a, b))]
        paths.append((int(path["name_start"]), int(path["name_end"]), path_start, len(steps), 0, 0))  # :99-103
    # chop.rs:106-134
    if links:
        for ln in p.links:
            f, t = int(ln["from_"]), int(ln["to"])
            fa, fb = seg_map[f >> 1]
            ta, tb = seg_map[t >> 1]
            nf = (fb - 1) if f & 1 == 0 else fa  # :111-116
            nt = ta if t & 1 == 0 else (tb - 1)  # :120-125
            new_links.append(((nf << 1) | (f & 1), (nt << 1) | (t & 1)))
    sg = np.zeros(len(segs), fo.SEG_DT)
    if segs:
        a = np.array(segs, dtype=np.uint64)
        sg["name"], sg["seq_start"], sg["seq_end"] = a[:, 0], a[:, 1], a[:, 2]
    pt = np.zeros(len(paths), fo.PATH_DT)
    for i, r in enumerate(paths):
        pt[i] = r
    lk = np.zeros(len(new_links), fo.LINK_DT)  # overlap = the empty alignment (0, 0), flatgfa.rs:494-500
    if new_links:
        a = np.array(new_links, dtype=np.uint32)
        lk["from_"], lk["to"] = a[:, 0], a[:, 1]
    return _store(p, sg, pt, lk, np.array(steps, dtype=np.uint32))


def seg_first(p: fo.Pools, c: int) -> np.ndarray:
    lens = (p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"].astype(np.int64))
    k = np.where(lens <= c, 1, (lens - 1) // c + 1)
    return np.concatenate([[0], np.cumsum(k)]).astype(np.int64)


def chop_fast(p: fo.Pools, c: int, links: bool = False) -> fo.Pools:
    """The same pools by np.repeat over the piece counts (no Python loop over steps or segments)."""
    if c <= 0:
        raise ValueError("max_size 0: the reference loops forever")
    st = p.segs["seq_start"].astype(np.int64)
    lens = p.segs["seq_end"].astype(np.int64) - st
    k = np.where(lens <= c, 1, (lens - 1) // c + 1)
    first = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    S2 = int(first[-1])
    old = np.repeat(np.arange(len(k)), k)
    piece = np.arange(S2, dtype=np.int64) - first[old]
    start = st[old] + piece * c
    end = np.where(piece == k[old] - 1, st[old] + lens[old], start + c)
    sg = np.zeros(S2, fo.SEG_DT)
    sg["name"], sg["seq_start"], sg["seq_end"] = np.arange(1, S2 + 1), start, end
    # the steps of every path, in path order
    b = p.paths["steps_start"].astype(np.int64)
    e = p.paths["steps_end"].astype(np.int64)
    n = e - b
    if len(n) and np.array_equal(b[1:], e[:-1]) and b[0] == 0:
        idx = np.arange(b[0], e[-1])
    else:
        idx = (np.repeat(b - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))).astype(np.int64)
    h = p.steps[idx].astype(np.int64)
    s = h >> 1
    if len(s) and s.max() >= len(k):
        raise IndexError("a step names a segment that is not there")
    kk = k[s]
    offs = np.concatenate([[0], np.cumsum(kk)]).astype(np.int64)
    rep = np.repeat(np.arange(len(h)), kk)
    pc = np.arange(int(offs[-1]), dtype=np.int64) - offs[rep]
    base, kr, bw = first[s][rep], kk[rep], (h[rep] & 1)
    steps = np.where(bw == 0, (base + pc) << 1, ((base + kr - 1 - pc) << 1) | 1).astype(np.uint32)
    pstart = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    pt = np.zeros(len(n), fo.PATH_DT)
    pt["name_start"], pt["name_end"] = p.paths["name_start"], p.paths["name_end"]
    pt["steps_start"], pt["steps_end"] = offs[pstart[:-1]], offs[pstart[1:]]
    lk = np.zeros(0, fo.LINK_DT)
    if links:
        nid = np.arange(S2, dtype=np.int64)
        intra = nid[piece < k[old] - 1]
        f, t = p.links["from_"].astype(np.int64), p.links["to"].astype(np.int64)
        fs, ts = f >> 1, t >> 1
        if len(f) and max(fs.max(), ts.max()) >= len(k):
            raise IndexError("a link names a segment that is not there")
        nf = np.where(f & 1 == 0, first[fs + 1] - 1, first[fs])
        nt = np.where(t & 1 == 0, first[ts], first[ts + 1] - 1)
        lk = np.zeros(len(intra) + len(f), fo.LINK_DT)
        lk["from_"] = np.concatenate([intra << 1, (nf << 1) | (f & 1)])
        lk["to"] = np.concatenate([(intra + 1) << 1, (nt << 1) | (t & 1)])
    return _store(p, sg, pt, lk, steps)


def pools_of(g) -> fo.Pools:
    """The pools of a pollen_amd FlatGFA."""
    return fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})


def same_pools(a: fo.Pools, b: fo.Pools) -> bool:
    return all(getattr(a, n).tobytes() == getattr(b, n).tobytes() for n in fo.POOL_ORDER)


def text(p: fo.Pools) -> bytes:
    """The GFA text the project's printer makes of these pools (through a .flatgfa file and flatgfa_load)."""
    import pollen_amd as pa
    fd, path = tempfile.mkstemp(suffix=".flatgfa")
    try:
        with os.fdopen(fd, "wb") as f:
            f.write(fo.dump_flatgfa(p))
        g = pa.load(path)
        out = g.gfa_text()
        g.close()
        return out
    finally:
        os.unlink(path)


def odgi_view(p: fo.Pools):
    """What slow_odgi's chop output holds of a graph: {segment name: sequence} and {path name: [handle text]}."""
    segs = {str(int(s["name"])): p.seq_data[int(s["seq_start"]):int(s["seq_end"])].tobytes().decode() for s in p.segs}
    names = [str(int(s["name"])) for s in p.segs]
    paths = {}
    for path in p.paths:
        nm = p.name_data[int(path["name_start"]):int(path["name_end"])].tobytes().decode()
        paths[nm] = [names[int(h) >> 1] + ("-" if int(h) & 1 else "+") for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]]
    return segs, paths


def parse_odgi_text(t: bytes):
    segs, paths = {}, {}
    for ln in t.decode().splitlines():
        f = ln.split("\t")
        if f[0] == "S":
            segs[f[1]] = f[2]
        elif f[0] == "P":
            paths[f[1]] = f[2].split(",") if f[2] else []
    return segs, paths
