"""A plain-Python restatement of the reference's inject (slow_odgi/slow_odgi/inject.py, `odgi inject`) over the pools of
oracle/flatgfa_oracle.py, in two forms that tests/test_inject_model.py pins to each other:

  inject_sequential   inject.py line by line: every BED line is handled on the graph the line before left, every cut
                      renumbers the segments behind it and rebuilds every path (chop_if_needed), and a new path is put
                      into the path dictionary in place.
  inject              the one-pass form that the library computes, rule by rule, each with the line
                      of the reference it restates.  The three cases where one pass cannot say what the dictionary update
                      does raise Refused; inject_sequential shows what the reference gives there.

A line is (path name, low, high, new name), names as bytes.  Segments are known by their index (new id i is named i + 1, as
slow_odgi needs them and chop.rs makes them).  Test infrastructure only."""
import numpy as np

import chop_model as cm
from oracle import flatgfa_oracle as fo


class Refused(Exception):
    """What the library answers FLATGFA_ERR_ARG for; .line is the index of the BED line."""

    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


# ---- the pools as plain lists, and back ----
def _read(p: fo.Pools):
    segs = [(int(s["seq_start"]), int(s["seq_end"])) for s in p.segs]
    paths = {}
    order = []
    for path in p.paths:
        nm = p.name_data[int(path["name_start"]):int(path["name_end"])].tobytes()
        paths[nm] = [int(h) for h in p.steps[int(path["steps_start"]):int(path["steps_end"])]]
        order.append(nm)
    assert len(paths) == len(order), "path names must be distinct for the model"
    return segs, paths


def _pools(p: fo.Pools, segs, paths, links) -> fo.Pools:
    """Header, seq_data and name_data from the input; names that the input lacks are appended to name_data in path order."""
    old = {}
    for path in p.paths:
        a, b = int(path["name_start"]), int(path["name_end"])
        old.setdefault(p.name_data[a:b].tobytes(), (a, b))
    name_data = bytearray(p.name_data.tobytes())
    sg = np.zeros(len(segs), fo.SEG_DT)
    for i, (a, b) in enumerate(segs):
        sg[i] = (i + 1, a, b, 0, 0)  # inject.py:71-77 names; no optional fields
    pt = np.zeros(len(paths), fo.PATH_DT)
    steps = []
    for i, (nm, hs) in enumerate(paths.items()):
        if nm in old:
            a, b = old[nm]
        else:
            a = len(name_data)
            name_data += nm
            b = len(name_data)
        pt[i] = (a, b, len(steps), len(steps) + len(hs), 0, 0)  # chop.py:56: overlaps are dropped
        steps += hs
    lk = np.zeros(len(links), fo.LINK_DT)
    for i, (f, t) in enumerate(links):
        lk[i] = (f, t, 0, 0)
    return fo.Pools(header=p.header, segs=sg, paths=pt, links=lk, steps=np.array(steps, dtype=np.uint32), seq_data=p.seq_data,
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(bytes(name_data), np.uint8),
                    optional_data=cm.E8(), line_order=cm.E8())


# ---- inject.py, line by line ----
def _where_chop(segs, steps, index):
    walk = 0
    for h in steps:  # inject.py:38-46
        if walk == index:
            return None
        length = segs[h >> 1][1] - segs[h >> 1][0]
        if walk + length > index:
            o = index - walk
            return h >> 1, (o if h & 1 == 0 else length - o)  # handle_pos, :24-28
        walk += length
    return None


def _chop_if_needed(segs, paths, name, index):
    target = _where_chop(segs, paths[name], index)
    if target is None:
        return segs, paths  # :57-58
    t, pos = target
    a, b = segs[t]
    new_segs = segs[:t] + [(a, a + pos), (a + pos, b)] + segs[t + 1:]  # :64-78
    legend = [(s, s + 1) if s < t else (s, s + 2) if s == t else (s + 1, s + 2) for s in range(len(segs))]
    new_paths = {}
    for nm, hs in paths.items():  # chop.py:46-58
        out = []
        for h in hs:
            fst, snd = legend[h >> 1]
            ids = list(range(fst, snd))
            out += [i << 1 for i in ids] if h & 1 == 0 else [(i << 1) | 1 for i in reversed(ids)]
        new_paths[nm] = out
    return new_segs, new_paths


def _track_path(segs, steps, low, high):
    walk, out = 0, []
    for h in steps:  # inject.py:10-21
        length = segs[h >> 1][1] - segs[h >> 1][0]
        if walk < low:
            walk += length
            continue
        if walk + length <= high:
            walk += length
            out.append(h)
        else:
            return out
    return out


def inject_sequential(p: fo.Pools, lines) -> fo.Pools:
    """inject.py:84-93.  No links: slow_odgi prints none (__main__.py:187)."""
    segs, paths = _read(p)
    for name, low, high, new in lines:
        if name in paths:  # :87
            segs, paths = _chop_if_needed(segs, paths, name, low)
            segs, paths = _chop_if_needed(segs, paths, name, high)  # :90
            paths[new] = _track_path(segs, paths[name], low, high)  # :91-92, in place: an old key keeps its place
    return _pools(p, segs, paths, [])


# ---- one pass ----
def locate(segs, steps, x):
    """The cut of line end x on a path (inject.py:24-46): (segment, position), or None when x is on a seam or past the end."""
    return _where_chop(segs, steps, x)


def cut_table(p: fo.Pools, lines):
    """{segment: sorted distinct cut positions} of the lines that are not skipped, and those lines."""
    segs, paths = _read(p)
    kept, fresh = [], set()
    for k, (name, low, high, new) in enumerate(lines):
        if name not in paths:
            if name in fresh:
                raise Refused(k, "its path is an earlier line's new name")  # (the reference finds the injected path)
            continue  # inject.py:87
        if new in paths:
            raise Refused(k, "the new name is a path of the graph")  # (the reference replaces that path where it stands)
        if new in fresh:
            raise Refused(k, "the new name was given by an earlier line")  # (the later one wins in the reference)
        fresh.add(new)
        kept.append((name, low, high, new))
    cuts = {}
    for name, low, high, _new in kept:
        for x in (low, high):
            c = locate(segs, paths[name], x)
            if c is not None:
                assert 0 < c[1] < segs[c[0]][1] - segs[c[0]][0]
                cuts.setdefault(c[0], set()).add(c[1])
    return {s: sorted(v) for s, v in cuts.items()}, kept


def inject(p: fo.Pools, lines, links: bool = False) -> fo.Pools:
    segs, paths = _read(p)
    cuts, kept = cut_table(p, lines)
    # segments: k distinct cuts make k + 1 segments, in old-segment order and by position (inject.py:49-81)
    new_segs, first = [], []
    for s, (a, b) in enumerate(segs):
        first.append(len(new_segs))
        edges = [0] + cuts.get(s, []) + [b - a]
        new_segs += [(a + lo, a + hi) for lo, hi in zip(edges[:-1], edges[1:])]
    first.append(len(new_segs))
    # old paths: a forward step becomes its pieces in order, a backward one the same reversed (chop.py:46-58)
    new_paths = {}
    for nm, hs in paths.items():
        out = []
        for h in hs:
            ids = range(first[h >> 1], first[(h >> 1) + 1])
            out += [i << 1 for i in ids] if h & 1 == 0 else [(i << 1) | 1 for i in reversed(ids)]
        new_paths[nm] = out
    # new paths: the steps from the first with start >= low up to the first with end > high (inject.py:6-21)
    for name, low, high, new in kept:
        hs = new_paths[name]
        ends = np.cumsum([new_segs[h >> 1][1] - new_segs[h >> 1][0] for h in hs]).tolist()
        starts = [0] + ends[:-1]
        lo = next((i for i, s in enumerate(starts) if s >= low), len(hs))
        hi = next((i for i in range(lo, len(hs)) if ends[i] > high), len(hs))
        new_paths[new] = list(hs[lo:hi])
    # links: none, or chop's rule (chop.rs:106-134)
    lk = []
    if links:
        for s in range(len(segs)):
            lk += [(i << 1, (i + 1) << 1) for i in range(first[s], first[s + 1] - 1)]
        for ln in p.links:
            f, t = int(ln["from_"]), int(ln["to"])
            nf = first[(f >> 1) + 1] - 1 if f & 1 == 0 else first[f >> 1]
            nt = first[t >> 1] if t & 1 == 0 else first[(t >> 1) + 1] - 1
            lk.append(((nf << 1) | (f & 1), (nt << 1) | (t & 1)))
    return _pools(p, new_segs, new_paths, lk)


def seg_first(p: fo.Pools, lines) -> np.ndarray:
    cuts, _ = cut_table(p, lines)
    k = np.array([len(cuts.get(s, [])) + 1 for s in range(len(p.segs))], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(k)]).astype(np.int64)


def bed_text(lines) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%s\n" % ln for ln in lines)


pools_of, same_pools, text, odgi_view, parse_odgi_text = cm.pools_of, cm.same_pools, cm.text, cm.odgi_view, cm.parse_odgi_text
