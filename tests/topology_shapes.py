"""Graphs for validate and degree (tests/topology_model.py restates the rules): the mid-size synthetic graph whose reference
output is pinned under tests/golden/topology/, and planted graphs sized by the constants of pollen_amd/csrc/topology_device.hip,
each with the answer derived by hand -- the records as (path, step) pairs -- so that a shape that is wrong in itself shows up
on the CPU (tests/test_topology_model.py runs every one through the model)."""
import os
import re
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

from oracle import flatgfa_oracle as fo
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the constants of topology_device.hip, restated here once (kernel_constants() reads them back from the source)
THREADS, PER, MAX_GRID, LINEAR = 256, 4, 2048, 16
TILE = THREADS * PER


def kernel_constants() -> dict:
    src = open(os.path.join(ROOT, "pollen_amd", "csrc", "topology_device.hip")).read()
    return {k: int(re.search(r"constexpr \w+ %s = (\d+);" % k, src).group(1)) for k in ("kThreads", "kPer", "kMaxGrid", "kLinear")}


def fwd(seg):
    return np.asarray(seg, np.uint32) << 1


def make_pools(n_segs: int, steps, spans, links) -> fo.Pools:
    """Segments named 1 .. n_segs of one base each; path k, named p<k>, walks steps[spans[k][0] : spans[k][1]]; links is a
    list of (from, to) handles."""
    segs = np.zeros(n_segs, fo.SEG_DT)
    segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, n_segs + 1), np.arange(n_segs), np.arange(1, n_segs + 1)
    names = [b"p%d" % k for k in range(len(spans))]
    ne = np.cumsum([len(n) for n in names]).astype(np.int64) if names else np.zeros(0, np.int64)
    paths = np.zeros(len(spans), fo.PATH_DT)
    if len(spans):
        paths["name_end"], paths["name_start"] = ne, ne - [len(n) for n in names]
        paths["steps_start"], paths["steps_end"] = [s[0] for s in spans], [s[1] for s in spans]
    lk = np.zeros(len(links), fo.LINK_DT)
    if len(links):
        arr = np.asarray(links, np.uint32).reshape(-1, 2)
        lk["from_"], lk["to"] = arr[:, 0], arr[:, 1]
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=np.frombuffer(b"VN:Z:1.0", np.uint8).copy(), segs=segs, paths=paths, links=lk,
                    steps=np.ascontiguousarray(steps, np.uint32), seq_data=np.frombuffer((b"ACGT" * (n_segs // 4 + 1))[:n_segs], np.uint8).copy(),
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(b"".join(names), np.uint8).copy(),
                    optional_data=z, line_order=z)


def gfa_text(p: fo.Pools) -> bytes:
    """S, P and L lines of pools whose segments all have a sequence and whose links have no overlap: what slow_odgi reads."""
    out = []
    seq = p.seq_data.tobytes()
    for s in p.segs:
        out.append(b"S\t%d\t%s" % (int(s["name"]), seq[int(s["seq_start"]):int(s["seq_end"])]))
    name = p.segs["name"]
    for k, path in enumerate(p.paths):
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])]
        out.append(b"P\t%s\t%s\t*" % (p.path_name(k), b",".join(b"%d%s" % (int(name[h >> 1]), b"-" if h & 1 else b"+") for h in st.tolist())))
    for l in p.links:
        f, t = int(l["from_"]), int(l["to"])
        out.append(b"L\t%d\t%s\t%d\t%s\t0M" % (int(name[f >> 1]), b"-" if f & 1 else b"+", int(name[t >> 1]), b"-" if t & 1 else b"+"))
    return b"\n".join(out) + b"\n"


def induced_links(p: fo.Pools, form_salt: int, drop_salt: int, drop_per_million: int) -> np.ndarray:
    """The distinct consecutive step pairs of p's paths, each written in one of its two equivalent forms (chosen by a hash of
    the pair), then the chain i+ -> (i + 1)+; a pair or chain link whose hash falls below drop_per_million is left out."""
    pairs = []
    for path in p.paths:
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])].astype(np.uint64)
        pairs.append((st[:-1] << np.uint64(32)) | st[1:])
    S = len(p.segs)
    chain = (fwd(np.arange(S - 1)).astype(np.uint64) << np.uint64(32)) | fwd(np.arange(1, S)).astype(np.uint64)
    keys = np.concatenate([np.unique(np.concatenate(pairs)) if pairs else np.zeros(0, np.uint64), chain])
    h = synth.mix64(keys ^ np.uint64(drop_salt))
    keys = keys[(h % np.uint64(1_000_000)) >= np.uint64(drop_per_million)]
    a, b = (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rev = (synth.mix64(keys ^ np.uint64(form_salt)) & np.uint64(1)).astype(bool)
    return np.stack([np.where(rev, b ^ 1, a), np.where(rev, a ^ 1, b)], axis=1).astype(np.uint32)


def with_links(p: fo.Pools, links: np.ndarray) -> fo.Pools:
    lk = np.zeros(len(links), fo.LINK_DT)
    lk["from_"], lk["to"] = links[:, 0], links[:, 1]
    q = fo.Pools(**{n: getattr(p, n) for n in fo.POOL_ORDER})
    q.links = lk
    return q


SYNTH_MID = dict(seed=11, S=8000, P=10, L=10000, model="pangenome", form_salt=0x51, drop_salt=0xD0, drop_per_million=4000)


def synth_mid() -> fo.Pools:
    """oracle/synth.py's pangenome of 8 000 segments and 10 paths of 10 000 steps, with the links its paths induce."""
    c = SYNTH_MID
    p = synth.pools(c["seed"], c["S"], c["P"], c["L"], c["model"])
    return with_links(p, induced_links(p, c["form_salt"], c["drop_salt"], c["drop_per_million"]))


# ---- planted graphs ----

@dataclass
class Shape:
    name: str
    what: str
    make: Callable[[], fo.Pools]
    missing: Optional[List[Tuple[int, int]]] = None  # the (path, step) of every record, in order; None: given by n_missing and last
    n_missing: Optional[int] = None
    last: Optional[Tuple[int, int]] = None

    def pools(self) -> fo.Pools:
        return self.make()


def chain_links(n):
    """i+ -> (i + 1)+ for the segments 0 .. n, and the way back round."""
    return [(int(fwd(i)), int(fwd((i + 1) % n))) for i in range(n)]


def planted(n_steps: int, at: List[int], how: str, spans=None, extra_segs: int = 0) -> fo.Pools:
    """Steps walk the ring of M segments forwards, except X (segment M) at every k of `at` and Y (segment M + 1) behind it.
    The ring, the way into X and the way out of Y are linked; X -> Y is linked forwards (how = "fwd"), only as its reverse
    complement Y- -> X- ("rev"), or not at all ("none")."""
    M = 97
    X, Y = int(fwd(M)), int(fwd(M + 1))
    steps = fwd(np.arange(n_steps) % M)
    links = chain_links(M)
    for k in at:
        steps[k], steps[k + 1] = X, Y
        if k > 0:
            links.append((int(steps[k - 1]), X))
        if k + 2 < n_steps:
            links.append((Y, int(fwd((k + 2) % M))))
    if how == "fwd":
        links.append((X, Y))
    elif how == "rev":
        links.append((Y ^ 1, X ^ 1))
    return make_pools(M + 2 + extra_segs, steps, spans if spans is not None else [(0, n_steps)], links)


SMALL_N = 3 * TILE + 5
EDGES = [PER - 1, 64 * PER - 1, TILE - 1, 2 * TILE - 1]  # the last step of a lane, of a wave, of the first two workgroups' tiles
ROUND = MAX_GRID * TILE  # the steps of one grid-stride round
BIG_N = ROUND + 300 * TILE + 7


def _hub():
    """Three hub handles whose rows are longer than, exactly at and one above the linear-probe threshold, filled in a shuffled
    order with duplicates; two-step paths look up the first and last entry of each row and just below and above them."""
    S = 10_200
    rows = {0: 5000, 2: LINEAR, 4: LINEAR + 1}  # hub handle -> distinct entries
    links, spans, steps, missing = [], [], [], []
    for hub, n in rows.items():
        t = 8 + 4 * np.arange(n)
        ent = np.concatenate([t, t[:3]]) if hub == 0 else t  # (duplicates would lengthen the two rows at the threshold)
        links += [(hub, int(x)) for x in ent]
        for probe, hit in ((t[0], True), (t[-1], True), (t[n // 2], True), (t[0] - 1, False), (t[-1] + 1, False), (t[n // 2] + 1, False),
                           (t[0] + 2, False)):
            if not hit:
                missing.append((len(spans), 0))
            spans.append((len(steps), len(steps) + 2))
            steps += [hub, int(probe)]
    order = np.random.default_rng(3).permutation(len(links))
    return make_pools(S, steps, spans, [links[i] for i in order]), missing


def _hub_pools():
    return _hub()[0]


def _short_paths():
    # long, 0, 1, 2 supported, 2 unsupported, 0, long, 1 -- the short ones inside one tile, X = 97, Y = 98
    M = 97
    a = fwd(np.arange(1500) % M).tolist()
    steps = a + [int(fwd(5))] + [int(fwd(3)), int(fwd(4))] + [int(fwd(M)), int(fwd(M + 1))] + a + [int(fwd(M + 1))]
    spans = [(0, 1500), (1500, 1500), (1500, 1501), (1501, 1503), (1503, 1505), (1505, 1505), (1505, 3005), (3005, 3006)]
    return make_pools(M + 2, steps, spans, chain_links(M))


def _boundary():
    # path 0 ends with X exactly at a tile's last step; path 1 begins with Y: X -> Y is no pair of any path
    p = planted(SMALL_N, [TILE - 1], "none", spans=[(0, TILE), (TILE, SMALL_N)])
    return p


def _overlap_gaps():
    # X at 2047, Y at 2048 of the pool.  p0 = [0, 2048) ends with X; p1 = [1000, 4000) holds the pair at its step 1047;
    # p2 = [2048, 3000) begins with Y; p3 = [4500, 5000) lies behind a gap; p4 = [200, 700) lies before p3 in the pool
    return planted(5000, [2047], "none", spans=[(0, 2048), (1000, 4000), (2048, 3000), (4500, 5000), (200, 700)])


def _all_missing():
    # no links: every pair of 13 paths of 4 001 steps is missing -- 52 000 records over 51 output tiles
    return make_pools(50, fwd(np.arange(13 * 4001) % 50), [(k * 4001, (k + 1) * 4001) for k in range(13)], [])


def _degree_hub():
    # segment 0: 70 000 link ends from duplicates of ten links (its row is sorted: 70 000 entries); segment 5: a self-loop and the
    # palindromic 5+ -> 5- in both spellings; p5 = 11-,10- is supported by the reverse complement of 10+ -> 11+
    links = [(0, 8 + 4 * (i % 10)) for i in range(70_000)] + [(10, 10), (10, 11), (11, 10), (20, 22), (20, 22)]
    return make_pools(50, [0, 8, 0, 9, 10, 10, 10, 11, 20, 22, 23, 21], [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12)], links)


def _rows(S: int):
    """S segments, so a row array of 2 S + 1 entries (one per handle, and the end of the last row) for the in-place scan.  Links
    lie in the rows on both sides of every edge of the row tiles named below and in the two topmost rows, 2 S - 2 and 2 S - 1
    (the only key of row 2 S - 1 is the palindrome (S-1)- -> (S-1)+), so a prefix that is off at any of them misplaces a row
    that a two-step path then looks up; one pair in a top row is left unsupported."""
    edges = [e for e in (TILE, 2 * TILE, (THREADS - 1) * TILE, THREADS * TILE) if e < 2 * S]  # (in handles: the first row of a tile)
    segs = sorted({s for e in edges for s in (e // 2 - 1, e // 2) if s + 1 < S} | {0, S - 2})
    top = int(fwd(S - 1))
    links = [(int(fwd(s)), int(fwd(s + 1))) for s in segs] + [(top ^ 1, top)]
    pairs = links + [(top, top), (top ^ 1, int(fwd(S - 2)) ^ 1)]  # (S-1)+ -> (S-1)+: none; (S-1)- -> (S-2)-: the reverse of a link
    steps = [h for pr in pairs for h in pr]
    return make_pools(S, steps, [(2 * k, 2 * k + 2) for k in range(len(pairs))], links), [(len(links), 0)]


# Row arrays whose last tile lacks one entry (2 S + 1 is odd and a tile even: a full last tile does not exist), whose last tile
# holds one entry, and of more tiles than the one workgroup of the spine takes in a round
ROWS = {"rows_last_tile_one_short": TILE // 2 - 1, "rows_last_tile_of_one": TILE // 2, "rows_past_a_spine_round": THREADS * TILE // 2 + 1}

SHAPES = [Shape("edge_%d_%s" % (k, how), "the pair (X, Y) with X the last step of a lane, a wave or a workgroup's tile: %s" % how,
                (lambda k=k, how=how: planted(SMALL_N, [k], how)), missing=[(0, k)] if how == "none" else [])
          for k in EDGES for how in ("none", "rev", "fwd")] + [
    Shape("grid_round_none", "X is the last step of the first grid-stride round, Y the first of the second",
          lambda: planted(BIG_N, [ROUND - 1], "none"), missing=[(0, ROUND - 1)]),
    Shape("grid_round_rev", "... supported only by the reversed link", lambda: planted(BIG_N, [ROUND - 1], "rev"), missing=[]),
    Shape("grid_round_paths", "several paths over more than one round, pairs missing at tile and round edges of the steps laid end to end",
          lambda: planted(BIG_N, [TILE - 1, ROUND - 1, ROUND + TILE - 1, BIG_N - 2], "none",
                          spans=[(0, 5), (5, 5), (5, ROUND - 3), (ROUND - 3, ROUND + 2 * TILE), (ROUND + 2 * TILE, BIG_N)]),
          missing=[(2, TILE - 1 - 5), (3, 2), (3, TILE + 2), (4, BIG_N - 2 - ROUND - 2 * TILE)]),
    Shape("path_ends_at_tile_edge", "a path ends with X at a tile's last step and the next begins with Y: nothing", _boundary, missing=[]),
    Shape("short_paths", "paths of 0, 1 and 2 steps between long ones", _short_paths, missing=[(4, 0)]),
    Shape("overlap_and_gaps", "spans that overlap, leave gaps and do not ascend", _overlap_gaps, missing=[(1, 1047)]),
    Shape("all_missing", "L = 0: N - P records", _all_missing, n_missing=13 * 4000, last=(12, 3999)),
    Shape("none_missing", "a ring walked three times round", lambda: planted(SMALL_N, [], "none"), missing=[]),
    Shape("hub_rows", "rows longer than, at and one above the linear-probe threshold", _hub_pools, missing=_hub()[1]),
    Shape("degree_hub", "a segment with more than 65 535 link ends, self-loops, duplicates", _degree_hub, missing=[(1, 0)]),
    Shape("no_segments", "S = 0: empty paths only", lambda: make_pools(0, [], [(0, 0), (0, 0)], []), missing=[]),
    Shape("no_paths", "P = 0", lambda: make_pools(9, [0, 2, 4], [], chain_links(9)), missing=[]),
    Shape("no_links", "L = 0 and one path", lambda: make_pools(9, [0, 2, 4], [(0, 3)], []), missing=[(0, 0), (0, 1)]),
    Shape("nothing", "S = P = L = 0", lambda: make_pools(0, [], [], []), missing=[]),
] + [Shape(name, "a row array of 2 * %d + 1 entries" % S, (lambda S=S: _rows(S)[0]), missing=_rows(S)[1]) for name, S in ROWS.items()]
BY_NAME = {s.name: s for s in SHAPES}
assert len(BY_NAME) == len(SHAPES)
BIG = {"grid_round_none", "grid_round_rev", "grid_round_paths", "rows_past_a_spine_round"}
