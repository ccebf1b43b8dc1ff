"""Seeded adversarial pools for the random differential slices of crush, flip, flatten, print and validate/degree, for the
tests only.  Where the geometry files plant one edge at a time, a case made here holds many of them at once: short and empty
segments inside the step in which an N run crosses a round, a clipped long name in the tile a line began before, hub rows
beside ties and palindromes.

    make(seed, profile)      the pools of one case; deterministic from the seed
    case_seed(seed, k)       the seed of case k of a slice's seed, so that a failure message can name make()'s arguments
    extras(seed, profile)    what a case sets beside its pools: flatten's NAME, the chunk hooks
    census(p, profile, ..)   how many instances of each class of CLASSES[profile] the pools hold, from the pools and the
                             kernels' constants alone -- conditions on the generator, never measurements of the library
    gfa_text(p)              the GFA text of a "text" pools, which the reference's Python reads

Every kernel constant is read back from the source text (the models' source_constants, topology_shapes.kernel_constants, and
kRounds of crush_device.hip here); the 64 that is left is the wavefront.  tests/test_random_pools.py holds the census
conditions on the CPU, tests/test_gpu_random_slices.py runs the cases on the device.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import crush_model as cm
import flatten_model as flm
import flip_model as fm
import print_model as pm
import print_shapes as ps
import topology_model as tm
import topology_shapes as ts
from oracle import flatgfa_oracle as fo
from oracle.synth import mix64

SEEDS = tuple(range(6))
CASES = {"crush": 30, "flip": 32, "flatten": 30, "print": 30, "topology": 30}
TEXT_SEEDS = (1, 3, 5)  # the three graphs per feature that the golden makers give the reference (their texts fit the folders' size)
WAVE = 64
N = cm.N


def _constants() -> Dict[str, Dict[str, int]]:
    with open(os.path.join(cm.CSRC, "crush_device.hip")) as f:
        rounds = re.search(r"constexpr uint32_t kRounds = (\d+);", f.read())
    assert rounds
    return {"crush": dict(cm.source_constants(), ROUNDS=int(rounds.group(1))), "flip": fm.source_constants(),
            "flat": flm.source_constants(), "topo": ts.kernel_constants()}


C = _constants()
CRUSH_TILE = C["crush"]["TILE"]
CRUSH_STEP = WAVE * C["crush"]["ROUNDS"]                     # the bytes of one crush_step
CRUSH_QUARTER = CRUSH_TILE // (C["crush"]["THREADS"] // WAVE)  # the stretch of a tile one wave walks
TEXT_TILE, LONG_NAME, WRAP = C["flat"]["TILE"], C["flat"]["LONG_NAME"], C["flat"]["WRAP"]
TOPO_PER, TOPO_LINEAR = C["topo"]["kPer"], C["topo"]["kLinear"]
TOPO_TILE = C["topo"]["kThreads"] * TOPO_PER
SHORT_ROW, LDS_ROW = C["flip"]["SHORT_ROW"], C["flip"]["LDS_ROW"]

CLASSES = {
    "crush": ["run over a round edge", "run over a step edge", "run over a wave-quarter edge", "run over a tile edge",
              "a run from a step's first byte on", "N-N over a segment seam", "64 or more segments begin in a step, empties among them",
              "first byte N behind another segment's N in the pool, at a step's first byte", "aliased bytes",
              "a tile's kept bytes begin off a 16-byte boundary"],
    "flip": ["turned", "not turned", "tied", "rows up to SHORT_ROW", "rows up to LDS_ROW", "rows past LDS_ROW",
             "a candidate that is an old link in the other spelling", "a pair walked by two turned paths",
             "links with an overlap other than 0M", "step spans not laid out in order"],
    "flatten": ["an empty segment at a FASTA tile's first base", "a BED line that begins in the tile before",
                "a clipped path name with more than LONG_NAME bytes in the tile", "a clipped path name with at most LONG_NAME bytes in the tile",
                "chunks"],
    "print": ["a long field clipped at a tile's end", "a long field clipped at a tile's start", "a chunk cut inside a path's steps",
              "line_order present", "line_order absent"],
    "topology": ["a looked-up row of length 0", "a looked-up row of length 1..LINEAR", "a looked-up row of length LINEAR+1",
                 "a looked-up row of hundreds", "a missing pair at a lane's last step", "a missing pair at a wave's last step",
                 "a missing pair at a tile's last step", "a pair supported only by the reverse complement", "a two-step path at a tile edge"],
}
PROFILES = tuple(CASES) + ("text",)


def case_seed(seed: int, k: int) -> int:
    return seed * 1000 + k


def _rng(seed: int, profile: str) -> np.random.Generator:
    return np.random.default_rng([seed, PROFILES.index(profile)])


def h(seg, back=False):
    return (int(seg) << 1) | (1 if back else 0)


def op(n: int, code: int = 0) -> int:
    return (n << 8) | code


# ---- assembling pools ----
def assemble(seg_spans, seq_data, step_pool, path_spans, path_names: Sequence[bytes], links=(), seg_names=None, header=b"") -> fo.Pools:
    """Pools of segments with these (start, end) spans into seq_data, paths with these spans into step_pool and these names
    (laid one behind another in name_data), links as (from, to, ops)."""
    spans = np.asarray(seg_spans, dtype=np.int64).reshape(-1, 2)
    segs = np.zeros(len(spans), fo.SEG_DT)
    segs["name"] = np.arange(1, len(spans) + 1) if seg_names is None else seg_names
    segs["seq_start"], segs["seq_end"] = spans[:, 0], spans[:, 1]
    pspans = np.asarray(path_spans, dtype=np.int64).reshape(-1, 2)
    paths = np.zeros(len(pspans), fo.PATH_DT)
    ne = np.cumsum([len(n) for n in path_names], dtype=np.int64) if len(path_names) else np.zeros(0, np.int64)
    paths["name_end"], paths["name_start"] = ne, ne - np.array([len(n) for n in path_names], dtype=np.int64)
    paths["steps_start"], paths["steps_end"] = pspans[:, 0], pspans[:, 1]
    al: List[int] = []
    lk = np.zeros(len(links), fo.LINK_DT)
    for i, (f, t, ops) in enumerate(links):
        lk[i] = (f, t, len(al), len(al) + len(ops))
        al += list(ops)
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=np.frombuffer(header, np.uint8).copy(), segs=segs, paths=paths, links=lk, steps=np.asarray(step_pool, dtype=np.uint32),
                    seq_data=np.asarray(seq_data, dtype=np.uint8), overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.asarray(al, dtype=np.uint32),
                    name_data=np.frombuffer(b"".join(path_names), np.uint8).copy(), optional_data=z, line_order=z)


class _Lens:
    """Segment lengths, with the laid-out offset the next one begins at."""

    def __init__(self):
        self.v: List[int] = []
        self.total = 0

    def add(self, xs) -> None:
        for x in np.atleast_1d(xs).tolist():
            self.v.append(int(x))
            self.total += int(x)

    def align(self, to: int) -> int:
        """One segment that ends on the next multiple of `to`; returns the index of the segment that then begins there."""
        self.add((-self.total) % to or to)
        return len(self.v)


def _names(rng, S: int) -> np.ndarray:
    """Numeric names, unique: dense, or sparse with gaps up to past 2^32."""
    if rng.random() < 0.4:
        return np.arange(1, S + 1, dtype=np.uint64)
    gaps = np.where(rng.random(S) < 0.1, rng.integers(1, 1 << 33, S), rng.integers(1, 12, S))
    return np.cumsum(gaps).astype(np.uint64)


def _lay_out(rng, lens: np.ndarray, mode: int):
    """Spans for these lengths: 0 one behind another, 1 in a shuffled order with gaps, 2 one behind another but a share of the
    segments aliasing a stretch that others own.  Returns (spans, pool length)."""
    lens = np.asarray(lens, dtype=np.int64)
    S = len(lens)
    if mode == 1:
        order = rng.permutation(S)
        gaps = np.where(rng.random(S) < 0.2, rng.integers(1, 4, S), 0)
        at = np.cumsum(lens[order] + gaps) - lens[order]
        start = np.zeros(S, np.int64)
        start[order] = at
        return np.stack([start, start + lens], axis=1), int((lens + gaps).sum())
    end = np.cumsum(lens)
    start = end - lens
    total = int(end[-1]) if S else 0
    if mode == 2 and total:
        for s in np.flatnonzero((rng.random(S) < 0.15) & (lens > 0)).tolist():
            start[s] = int(rng.integers(0, total - lens[s] + 1))
        twins = np.flatnonzero(lens > 3)
        for a, b in zip(twins[:-1:7].tolist(), twins[1::7].tolist()):  # b inside a's stretch, or a's own
            if lens[b] <= lens[a]:
                start[b] = start[a] + int(rng.integers(0, lens[a] - lens[b] + 1))
    return np.stack([start, start + lens], axis=1), total


def _acgt(rng, n: int) -> np.ndarray:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()


def _step_pool(rng, arrs: List[np.ndarray], mode: int, n_handles: int):
    """The paths' steps in one pool: 0 one behind another, 1 in a shuffled order with gaps of steps no path walks.  Returns
    (pool, spans)."""
    P = len(arrs)
    order = np.arange(P) if mode == 0 else rng.permutation(P)
    pool, spans = [], [None] * P
    at = 0
    for i in order.tolist():
        if mode and rng.random() < 0.3 and n_handles:
            junk = rng.integers(0, n_handles, int(rng.integers(1, 5))).astype(np.uint32)
            pool.append(junk)
            at += len(junk)
        spans[i] = (at, at + len(arrs[i]))
        pool.append(np.asarray(arrs[i], dtype=np.uint32))
        at += len(arrs[i])
    return (np.concatenate(pool) if pool else np.zeros(0, np.uint32)), spans


def _path_names(rng, P: int, lengths: Sequence[int]) -> List[bytes]:
    """Letters; path k's name is lengths[k % len(lengths)] long, and ends in its number where that fits."""
    out = []
    for k in range(P):
        n = int(lengths[k % len(lengths)])
        body = bytes(rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8))
        tag = b"%d" % k
        out.append(body[:n - len(tag)] + tag if n > len(tag) else body)
    return out


def induced(arrs: Sequence[np.ndarray], salt: int, drop_per_million: int) -> List[Tuple[int, int]]:
    """The distinct consecutive step pairs of these paths, each in one of its two spellings (by a hash of the pair), a
    fraction dropped: topology_shapes.induced_links without its chain."""
    pairs = [(np.asarray(a[:-1], np.uint64) << np.uint64(32)) | np.asarray(a[1:], np.uint64) for a in arrs if len(a) > 1]
    if not pairs:
        return []
    keys = np.unique(np.concatenate(pairs))
    keys = keys[(mix64(keys ^ np.uint64(salt * 2 + 1)) % np.uint64(1_000_000)) >= np.uint64(drop_per_million)]
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rev = (mix64(keys ^ np.uint64(salt * 2)) & np.uint64(1)).astype(bool)
    return list(zip(np.where(rev, b ^ 1, a).tolist(), np.where(rev, a ^ 1, b).tolist()))


def _walk(rng, n: int, lo: int, hi: int, back: float, local: bool = True) -> np.ndarray:
    """n steps over the segments [lo, hi): neighbours mostly, so that pairs come again; a share `back` backward."""
    if n == 0:
        return np.zeros(0, np.uint32)
    if local:
        seg = lo + (int(rng.integers(0, hi - lo)) + np.cumsum(rng.integers(-2, 4, n))) % (hi - lo)
    else:
        seg = rng.integers(lo, hi, n)
    return ((seg.astype(np.int64) << 1) | (rng.random(n) < back)).astype(np.uint32)


# ---- crush ----
def _plant_runs(rng, pool: np.ndarray, at_of: np.ndarray, total: int, edges: Sequence[Tuple[int, int]]) -> None:
    """N runs in laid-out coordinates (at_of maps them to the pool): across multiples of every edge, and anywhere."""
    def run(lo, hi):
        pool[at_of[max(lo, 0):min(hi, total)]] = N
    for e, most in edges:
        ms = np.arange(e, total, e)
        for m in (ms if len(ms) <= most else rng.choice(ms, most, replace=False)).tolist():
            a, b = [(int(rng.integers(1, 6)), int(rng.integers(1, 6))), (0, int(rng.integers(1, 6))), (int(rng.integers(1, 6)), 0)][int(rng.integers(0, 4)) % 3]
            run(m - a, m + b)  # across the edge, and now and then from it on or up to it
    for _ in range(15):
        a = int(rng.integers(0, max(total, 1)))
        run(a, a + int(rng.integers(1, 10)))
    if total > 400:
        a = int(rng.integers(0, total - 400))
        run(a, a + int(rng.integers(70, 300)))


def _crush(rng, k: int) -> fo.Pools:
    T, STEP, Q = CRUSH_TILE, CRUSH_STEP, CRUSH_QUARTER
    L = _Lens()
    seams: List[int] = []  # segments that begin on a seam of the walk

    def tens():
        L.add(rng.integers(10, 61, int(rng.integers(3, 30))))

    def empties():
        L.add(np.zeros(int(rng.integers(1, 21)), np.int64))

    def shorts(n):
        L.add(rng.choice([0, 1, 1, 2, 2, 3], int(n)))

    def seam(to):
        seams.append(L.align(to))
        L.add(int(rng.integers(1, 50)))

    def crowded(aligned):  # more than WAVE segments begin inside one step
        if aligned:
            seams.append(L.align(STEP))
        else:
            L.add(int(rng.integers(1, STEP)))
        shorts(rng.integers(WAVE + 6, 2 * WAVE))

    blocks = [tens, empties, lambda: seam(WAVE), lambda: crowded(True), lambda: crowded(False), lambda: seam(STEP), tens, lambda: shorts(rng.integers(5, 40)),
              empties, lambda: seam(STEP), tens]
    for i in rng.permutation(len(blocks)).tolist():
        blocks[i]()
    L.add(T - L.total % T + int(rng.integers(50, T // 2)))  # a long one over the next tile edge, and over wave quarters
    tens()
    seam(Q)
    crowded(True)
    empties()
    seam(T)
    tens()
    if k % 5 == 0:
        L.add(T + int(rng.integers(1, 300)))  # longer than a tile
        shorts(30)
    lens = np.array(L.v, dtype=np.int64)
    spans, pool_len = _lay_out(rng, lens, k % 3)
    pool = _acgt(rng, pool_len)
    p = assemble(spans, pool, [], [], [], seg_names=_names(rng, len(lens)))
    _, _, seg, _ = cm.laid_out(p)
    legend = np.concatenate([[0], np.cumsum(lens)])
    at_of = spans[seg, 0] + (np.arange(L.total) - legend[seg])
    _plant_runs(rng, pool, at_of, L.total, [(WAVE, 8), (STEP, 6), (Q, 8), (T, 8)])
    # N on both sides of a seam: at the planted seams and at some others; the pool byte before a seam segment is N as well
    full = np.flatnonzero(lens > 0)
    for s in seams + rng.choice(full, 12).tolist():
        if s >= len(lens) or lens[s] == 0:
            continue
        before = full[full < s]
        if len(before):
            pool[spans[before[-1], 1] - 1] = N
        pool[spans[s, 0]] = N
        if s in seams and spans[s, 0] > 0:
            pool[spans[s, 0] - 1] = N
    return p


def census_crush(p: fo.Pools) -> Dict[str, int]:
    T, STEP, Q = CRUSH_TILE, CRUSH_STEP, CRUSH_QUARTER
    b, first, _, lens = cm.laid_out(p)
    total = len(b)
    is_n = b == N
    cont = np.zeros(total, bool)  # the byte goes on an N run of its segment: crush drops it
    cont[1:] = is_n[1:] & is_n[:-1] & ~first[1:]
    at = np.flatnonzero(cont)
    leg = np.concatenate([[0], np.cumsum(lens)])[:-1]
    base = np.arange(0, total, STEP)
    ws = np.searchsorted(leg, base, side="right") - 1
    we = np.searchsorted(leg, np.minimum(base + STEP, total) - 1, side="right") - 1
    n_empty = np.concatenate([[0], np.cumsum(lens == 0)])
    crowded = (we - ws >= WAVE - 1) & (n_empty[we + 1] - n_empty[ws] > 0)
    start = p.segs["seq_start"].astype(np.int64)
    cover = np.zeros(len(p.seq_data) + 1, np.int64)
    np.add.at(cover, start, 1)
    np.add.at(cover, p.segs["seq_end"].astype(np.int64), -1)
    cover = np.cumsum(cover)[:-1]
    s = np.flatnonzero((lens > 0) & (leg % STEP == 0) & (leg > 0) & (start > 0))
    s = s[(p.seq_data[start[s]] == N) & (p.seq_data[start[s] - 1] == N) & (cover[start[s] - 1] > 0)]
    kept_before = np.concatenate([[0], np.cumsum(~cont)])
    tiles = np.arange(T, total, T)
    values = [int(((at % WAVE == 0) & (at % STEP != 0)).sum()), int(((at % STEP == 0) & (at % Q != 0)).sum()), int(((at % Q == 0) & (at % T != 0)).sum()),
              int((at % T == 0).sum()), int((is_n[base[1:]] & ~is_n[base[1:] - 1] & ~first[base[1:]]).sum()),
              int((first[1:] & is_n[1:] & is_n[:-1]).sum()), int(crowded.sum()), len(s), int((cover > 1).sum()),
              int((kept_before[tiles] % 16 != 0).sum())]
    return dict(zip(CLASSES["crush"], values))


# ---- flip ----
OVERLAPS = [[op(0)]] * 6 + [[], [op(5)], [op(3), op(1, 2)], [op(0), op(0)]]


def _spell(pairs, rng, drop: float):
    """(from, to, ops): each pair in one of its spellings, a fraction dropped, overlaps of none, one and several ops."""
    out = []
    for a, b in pairs:
        if rng.random() < drop:
            continue
        out.append((a, b, OVERLAPS[int(rng.integers(0, len(OVERLAPS)))]))
    return out


def _flip(rng, k: int) -> fo.Pools:
    big = k % 4 == 3
    S = int(rng.integers(40, 90 if big else 160))
    lens = rng.choice([0, 1, 1, 2, 3, 5, 12, 30], S)
    lens[:4] = [3, 1, 2, 1]
    arrs: List[np.ndarray] = []
    for _ in range(int(rng.integers(2, 4) if big else rng.integers(4, 9))):
        arrs.append(_walk(rng, int(rng.choice([3, 17, 64, 130, 300])), 4, S, float(rng.choice([0, 0.1, 0.5, 0.9, 1.0]))))
    w = _walk(rng, int(rng.integers(1, 40)), 4, S, 0.5)
    arrs.append(np.concatenate([w, w ^ 1]))                      # tied, whatever it weighs
    arrs.append(np.array([h(5), h(5, True)], np.uint32))         # tied over one segment
    twin = _walk(rng, int(rng.integers(2, 60)), 4, S, 1.0)
    arrs += [twin, twin.copy(), twin[::-1] ^ 1]                  # turned twice, and as it will be
    arrs += [np.zeros(0, np.uint32), _walk(rng, 1, 4, S, 1.0), _walk(rng, 2, 4, S, 1.0), np.zeros(0, np.uint32), _walk(rng, 2, 4, S, 0.0)]
    arrs.append(np.array([h(6, True), h(6), h(7, True), h(7, True)], np.uint32))  # turns into 7+,7+,6-,6+: a self-loop and a palindrome
    # hub rows: a turned path whose new steps are j+, k1, j+, k2, .. -- r keys with the high handle j+ and r - 1 with j-
    rs = [SHORT_ROW + int(rng.integers(-2, 4)), int(rng.integers(SHORT_ROW + 2, 700))]
    if big:
        rs.append(LDS_ROW + [1, -1, 2, 0, 3, 1, 2, 3][(k // 4) % 8])
    links = _spell(induced(arrs, k, 0), rng, 0.3)  # (not from the hub paths: their rows hold r keys and no more)
    for j, r in enumerate(rs):
        new = np.full(2 * r, h(j), np.uint32)
        new[1::2] = rng.integers(4, S, r) << 1
        arrs.append(new[::-1] ^ 1)
    order = rng.permutation(len(arrs))
    arrs = [arrs[i] for i in order.tolist()]
    pool, spans = _step_pool(rng, arrs, k % 3 and 1, 2 * S)
    if k % 3 == 2 and len(pool) > 10:  # shared and overlapping spans
        a = int(rng.integers(0, len(pool) - 5))
        spans += [spans[0], (a, a + int(rng.integers(1, min(200, len(pool) - a))))]
    links += links[:10] + [(b ^ 1, a ^ 1, ops) for a, b, ops in links[10:20]]
    links += [(h(9), h(9), [op(0)]), (h(10), h(10, True), [op(0)]), (h(10), h(10, True), []), (h(7), h(7), [op(0)])]
    links += [(int(a), int(b), [op(0)]) for a, b in rng.integers(0, 2 * S, (10, 2)).tolist()]
    links = [links[i] for i in rng.permutation(len(links)).tolist()]
    end = np.cumsum(lens)
    names = _path_names(rng, len(spans), [3, 0, 1, 9, 2, 40])
    return assemble(np.stack([end - lens, end], axis=1), np.full(int(end[-1]), 65, np.uint8), pool, spans, names, links, seg_names=_names(rng, S))


def census_flip(p: fo.Pools) -> Dict[str, int]:
    w = [fm.weigh(p, i) for i in range(len(p.paths))]
    n_steps = (p.paths["steps_end"].astype(np.int64) - p.paths["steps_start"]).tolist()
    t = fm.turned(p)
    rows = list(fm.row_sizes(p).values())
    old = set(fm.old_links(p))
    steps = fm.new_steps(p, t)
    cand = fm.candidates(steps, t)
    other = sum(1 for a, b in cand if (b ^ 1, a ^ 1) != (a, b) and (b ^ 1, a ^ 1, (0,)) in old and (a, b, (0,)) not in old)
    seen: Dict[Tuple[int, int], int] = {}
    for i, st in enumerate(steps):
        if t[i]:
            for key in {min((int(a), int(b)), (int(b) ^ 1, int(a) ^ 1)) for a, b in zip(st[:-1], st[1:])}:
                seen[key] = seen.get(key, 0) + 1
    al = p.alignment
    ovl = sum(1 for r in p.links if int(r["ov_end"]) > int(r["ov_start"]) and al[int(r["ov_start"]):int(r["ov_end"])].tolist() != [0])
    begin = np.concatenate([[0], p.paths["steps_end"][:-1].astype(np.int64)]) if len(p.paths) else np.zeros(0, np.int64)
    values = [int(t.sum()), sum(1 for f, r in w if r < f), sum(1 for (f, r), n in zip(w, n_steps) if f == r and n),
              sum(1 for n in rows if 2 <= n <= SHORT_ROW), sum(1 for n in rows if SHORT_ROW < n <= LDS_ROW), sum(1 for n in rows if n > LDS_ROW),
              other, sum(1 for n in seen.values() if n > 1), ovl, int((p.paths["steps_start"].astype(np.int64) != begin).sum())]
    return dict(zip(CLASSES["flip"], values))


# ---- validate and degree ----
def _topology(rng, k: int) -> fo.Pools:
    T, PER, LIN = TOPO_TILE, TOPO_PER, TOPO_LINEAR
    S = int(rng.integers(460, 700))
    X, Y = h(S - 2), h(S - 1)  # a pair no link supports
    lo, hi = 4, S - 2          # the walks' segments; 0 .. 3 are the hubs
    arrs: List[np.ndarray] = []
    walks: List[int] = []

    def walk(n):
        a = _walk(rng, n, lo, hi, 0.15)
        for at in rng.integers(0, max(n - 2, 1), 3).tolist():
            if n > 8:
                a[at + 1] = a[at] ^ np.uint32(rng.integers(0, 2))  # a self-loop, or the palindromic x+ -> x-
        walks.append(len(arrs))
        arrs.append(a)

    def short():
        arrs.append(_walk(rng, int(rng.integers(0, 3)), lo, hi, 0.5))

    walk(int(rng.integers(300, 900)))
    short()
    # hub rows and the two-step paths that look into them
    rows = {h(0): int(rng.integers(1, LIN + 1)), h(1): LIN + 1, h(2): int(rng.integers(100, 400)), h(3): LIN}
    hub_links: List[Tuple[int, int]] = []
    for hub, n in rows.items():
        t = (rng.choice(np.arange(lo, hi), n, replace=False) << 1) | rng.integers(0, 2, n)
        ent = np.concatenate([t, t[:3]]) if n > LIN + 1 else t  # (duplicates would lengthen the rows at the threshold)
        hub_links += [(hub, int(x)) for x in ent]
        for probe in (int(t[0]), int(t[-1]), int(t[n // 2]), int(t[0]) ^ 1, int(np.sort(t)[n // 2]) + 2):
            arrs.append(np.array([hub, probe], np.uint32))
        arrs.append(np.array([int(t[n // 2]) ^ 1, hub ^ 1], np.uint32))  # supported by the reverse complement alone
    walk(int(rng.integers(100, 700)))
    short()
    # a two-step path whose first step is a tile's last: a walk in front of it fills the tile
    done = sum(len(a) for a in arrs)
    walk((T - 1 - done) % T or T)
    arrs.append(np.array([X, Y], np.uint32) if k % 2 else _walk(rng, 2, lo, hi, 0.2))
    short()
    while sum(len(a) for a in arrs) < 2 * T + T // 2:
        walk(int(rng.integers(50, 600)))
        short()
    # (X, Y) planted where the first is the last step of a lane, a wave, a tile of the paths laid end to end
    pstart = np.concatenate([[0], np.cumsum([len(a) for a in arrs])])
    for i in walks:
        a, at0 = arrs[i], int(pstart[i])
        for period in (PER, WAVE * PER, T):
            js = [j for j in range(at0, at0 + len(a) - 1) if j % period == period - 1]
            for j in (js if period > PER else rng.choice(js, min(3, len(js)), replace=False).tolist() if js else []):
                a[j - at0], a[j - at0 + 1] = X, Y
    pool, spans = _step_pool(rng, arrs, k % 3 and 1, 2 * S)
    if k % 3 == 2:  # windows of the pool behind the others: shared and overlapping spans
        a = int(rng.integers(0, len(pool) - 50))
        spans += [spans[walks[0]], (a, a + int(rng.integers(2, 50)))]
    pairs = [pr for pr in induced([arrs[i] for i in walks], k, 30_000) if pr not in ((X, Y), (Y ^ 1, X ^ 1))]
    links = pairs + pairs[:20] + hub_links
    links = [(a, b, []) for a, b in (links[i] for i in rng.permutation(len(links)).tolist())]
    names = _path_names(rng, len(spans), [4, 6, 5])
    return assemble(np.stack([np.arange(S), np.arange(1, S + 1)], axis=1), _acgt(rng, S), pool, spans, names, links, seg_names=_names(rng, S),
                    header=b"VN:Z:1.0")


def canon(a: int, b: int) -> Tuple[int, int]:
    return min((a, b), (b ^ 1, a ^ 1))


def census_topology(p: fo.Pools) -> Dict[str, int]:
    T, PER, LIN = TOPO_TILE, TOPO_PER, TOPO_LINEAR
    have = set(zip(p.links["from_"].tolist(), p.links["to"].tolist()))
    row: Dict[int, int] = {}
    for f, t in zip(p.links["from_"].tolist(), p.links["to"].tolist()):
        hi = canon(f, t)[0]
        row[hi] = row.get(hi, 0) + 1
    looked = {"0": 0, "few": 0, "edge": 0, "many": 0, "other": 0}
    rev_only = two_step = 0
    n_steps = p.paths["steps_end"].astype(np.int64) - p.paths["steps_start"]
    pstart = np.concatenate([[0], np.cumsum(n_steps)])
    for i, path in enumerate(p.paths):
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])].tolist()
        two_step += len(st) == 2 and pstart[i] % T == T - 1
        for a, b in zip(st[:-1], st[1:]):
            n = row.get(canon(a, b)[0], 0)
            looked["0" if n == 0 else "few" if n <= LIN else "edge" if n == LIN + 1 else "many" if n >= 100 else "other"] += 1
            rev_only += (a, b) not in have and (b ^ 1, a ^ 1) in have
    r = tm.validate(p)
    at = pstart[r["path"].astype(np.int64)] + r["step"].astype(np.int64)
    values = [looked["0"], looked["few"], looked["edge"], looked["many"], int((at % PER == PER - 1).sum()),
              int((at % (WAVE * PER) == WAVE * PER - 1).sum()), int((at % T == T - 1).sum()), int(rev_only), int(two_step)]
    return dict(zip(CLASSES["topology"], values))


# ---- flatten ----
def _flatten(rng, k: int) -> fo.Pools:
    T = TEXT_TILE
    q = T  # byte q of the FASTA's body is tile 1's first; it is base q - q // (WRAP + 1) unless it is a newline
    assert q % (WRAP + 1) != WRAP
    b1 = q - q // (WRAP + 1)
    L = _Lens()
    L.add(rng.integers(10, 61, int(rng.integers(3, 30))))
    L.add(rng.choice([0, 1, 1, 2, 2, 3], int(rng.integers(20, 300))))
    L.add(np.zeros(int(rng.integers(1, 9)), np.int64))
    L.add(int(rng.integers(b1 // 3, b1 // 2)))
    L.add(rng.integers(0, 200, int(rng.integers(2, 12))))
    L.add(b1 - L.total)                                    # ends where tile 1 begins
    L.add(np.zeros(int(rng.integers(1, 9)), np.int64))     # empty ones at tile 1's first base
    L.add(rng.choice([0, 1, 2, 3, 40, 300], int(rng.integers(20, 80))))
    lens = np.array(L.v, dtype=np.int64)
    S = len(lens)
    spans, pool_len = _lay_out(rng, lens, k % 3)
    pool = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, pool_len)].copy()
    # paths: names of 0, 1 and around LONG_NAME bytes, of a few hundred, and one longer than a tile
    sizes = [0, 1, LONG_NAME - 1, LONG_NAME, LONG_NAME + 1, int(rng.integers(100, 400)), 3, int(rng.integers(70, 200))]
    counts = [int(rng.integers(0, 3)), int(rng.integers(1, 40)), 60, 70, 80, int(rng.integers(100, 250)), 0, int(rng.integers(100, 250))]
    if k % 2 == 0:
        sizes.append(T + int(rng.integers(1, 200)))
        counts.append(int(rng.integers(2, 6)))
    order = rng.permutation(len(sizes)).tolist()
    arrs = [_walk(rng, counts[i], 0, S, 0.3, local=False) for i in order]
    step_pool, pspans = _step_pool(rng, arrs, k % 3 and 1, 2 * S)
    if k % 3 == 2:
        pspans += [pspans[0], (3, 40)]
    names = [bytes(rng.integers(ord("A"), ord("Z") + 1, sizes[i], dtype=np.uint8)) for i in order] + [b"twin", b"window"][:len(pspans) - len(order)]
    return assemble(spans, pool, step_pool, pspans, names, seg_names=_names(rng, S))


def _bed_lines(p: fo.Pools, nm: bytes):
    """(length, where the path name begins in the line, the name's length) of every BED line."""
    leg = flm.legend(p)
    out = []
    for path in p.paths:
        n = int(path["name_end"]) - int(path["name_start"])
        for rank, hd in enumerate(p.steps[int(path["steps_start"]):int(path["steps_end"])].tolist()):
            lead = len(nm) + 1 + len(str(leg[hd >> 1])) + 1 + len(str(leg[(hd >> 1) + 1])) + 1
            out.append((lead + n + 3 + len(str(rank)) + 1, lead, n))
    return out


def _pieces(start: int, end: int, tile: int) -> List[int]:
    """The bytes of [start, end) in each tile it touches."""
    return [min(end, (t + 1) * tile) - max(start, t * tile) for t in range(start // tile, (end - 1) // tile + 1)] if end > start else []


def census_flatten(p: fo.Pools, nm: bytes, chunk: Optional[int]) -> Dict[str, int]:
    T = TEXT_TILE
    leg = np.array(flm.legend(p), dtype=np.int64)
    body = flm.fasta_body_len(int(leg[-1]))
    empty_first = 0
    for q in range(T, body - 1, T):
        if q % (WRAP + 1) != WRAP:
            b = q - q // (WRAP + 1)
            empty_first += int(((leg[:-1] == b) & (leg[1:] == b)).sum())
    lines = _bed_lines(p, nm)
    per = chunk or C["flat"]["CHUNK_LINES"]
    before = clip_long = clip_short = 0
    for c0 in range(0, len(lines), per):
        at = 0
        for n, lead, name in lines[c0:c0 + per]:
            before += at // T != (at + n - 1) // T
            cut = _pieces(at + lead, at + lead + name, T)
            if len(cut) > 1:
                clip_long += sum(1 for x in cut if x > LONG_NAME)
                clip_short += sum(1 for x in cut if x <= LONG_NAME)
            at += n
    n_chunks = -(-len(lines) // per)
    return dict(zip(CLASSES["flatten"], [empty_first, before, clip_long, clip_short, n_chunks if chunk and n_chunks > 1 else 0]))


# ---- print ----
def _cigar(rng, letters: bytes) -> bytes:
    if rng.random() < 0.7:
        return b"0M"
    return b"".join(b"%d%c" % (int(rng.integers(0, 256)), letters[int(rng.integers(0, len(letters)))]) for _ in range(int(rng.integers(1, 5))))


def _print(rng, k: int) -> fo.Pools:
    T = TEXT_TILE
    letters = b"MNDI" if k % 2 == 0 else b"MN"  # (the printer writes D for I and I for D, print.rs:18-19: odd cases are parsed back)
    S = int(rng.integers(200, 400))
    names = _names(rng, S).tolist()
    seq_len = rng.choice([1, 3, 9, LONG_NAME - 1, LONG_NAME, LONG_NAME + 1, 150, 400], S)
    seq_len[int(rng.integers(0, S))] = 2000
    if k % 5 == 0:
        seq_len[int(rng.integers(0, S))] = T + int(rng.integers(1, 500))
    s_lines = []
    for i in range(S):
        ln = b"S\t%d\t%s" % (names[i], _acgt(rng, int(seq_len[i])).tobytes())
        u = rng.random()
        if u < 0.15:
            ln += b"\tLN:i:%d" % seq_len[i]
        elif u < 0.3:
            ln += b"\tLN:i:%d\tzz:Z:%s" % (seq_len[i], bytes(rng.integers(ord("a"), ord("z") + 1, int(rng.integers(50, 300)), dtype=np.uint8)))
        s_lines.append(ln)
    p_lines, arrs = [], []
    pnames = _path_names(rng, int(rng.integers(3, 9)), [1, 5, LONG_NAME, LONG_NAME + 1, 200, LONG_NAME + 2, 30, 90])
    for i, pn in enumerate(pnames):
        st = _walk(rng, int(rng.choice([1, 2, 7, 60, 300])), 0, S, 0.3)
        arrs.append(st)
        ovl = b"*" if i % 3 or len(st) < 2 else b",".join(_cigar(rng, letters) for _ in range(len(st) - 1))
        p_lines.append(b"P\t%s\t%s\t%s" % (pn, b",".join(b"%d%s" % (names[x >> 1], b"-" if x & 1 else b"+") for x in st.tolist()), ovl))
    pairs = induced(arrs, k, 200_000) + [tuple(x) for x in rng.integers(0, 2 * S, (20, 2)).tolist()]
    l_lines = [b"L\t%d\t%s\t%d\t%s\t%s" % (names[a >> 1], b"-" if a & 1 else b"+", names[b >> 1], b"-" if b & 1 else b"+", _cigar(rng, letters))
               for a, b in pairs]
    header = [[], [b"H\tVN:Z:1.0"], [b"H\tVN:Z:1.0\tzz:Z:" + bytes(rng.integers(ord("a"), ord("z") + 1, int(rng.integers(60, 300)), dtype=np.uint8))]][k % 3]
    lines = header + s_lines + p_lines + l_lines
    if k % 2:  # any order: P and L before their S, the header in the middle
        lines = [lines[i] for i in rng.permutation(len(lines)).tolist()]
    p = fo.parse_gfa(b"\n".join(lines) + b"\n")
    return ps.normalized_pools(p) if (k // 2) % 2 else p


def census_print(p: fo.Pools, chunk: Optional[int]) -> Dict[str, int]:
    T = TEXT_TILE
    text = pm.gfa(p)
    sizes = ps.item_sizes(text)
    item_at = np.concatenate([[0], np.cumsum(sizes)])
    per = chunk or len(sizes)
    chunk_at = item_at[0:len(sizes):per]  # the byte every chunk begins at
    at_end = at_start = 0
    for _kind, a, b in ps.long_fields(text):
        c0 = int(chunk_at[np.searchsorted(chunk_at, a, side="right") - 1])
        cut = _pieces(a - c0, b - c0, T)
        if len(cut) > 1:
            at_end += cut[0] > LONG_NAME
            at_start += cut[-1] > LONG_NAME
    inside = 0
    if chunk:
        for (first, n), ln in zip(ps.line_items(text), text[:-1].split(b"\n")):
            inside += ln[:1] == b"P" and any(first < c < first + n for c in range(-(-first // chunk) * chunk, first + n, chunk))
    has = int(len(p.line_order) > 0)
    return dict(zip(CLASSES["print"], [int(at_end), int(at_start), int(inside), has, 1 - has]))


# ---- what the reference's Python reads ----
def _text(rng, k: int) -> fo.Pools:
    """At most 140 segments and 450 steps (the reference's output is committed, and no larger than its folder's fixtures):
    spans one behind another, no empty segment, unique path names without blanks, no path without steps, link overlaps of
    one M op: what mygfa parses.  N runs at segment ends and starts, ties, palindromes,
    self-loops, duplicate links in both spellings and a hub row past the linear-probe threshold are kept; of the palindromic
    links x+ -> x- is, and x- -> x+ is not (neither as a link nor as a pair of steps, which flip would make one)."""
    S = int(rng.integers(60, 140))
    lens = rng.choice([1, 1, 2, 3, 7, 30, 60], S)
    end = np.cumsum(lens)
    spans = np.stack([end - lens, end], axis=1)
    pool = _acgt(rng, int(end[-1]))
    for s in rng.choice(S, 30).tolist():  # N runs at both ends, over whole segments, N on both sides of a seam
        a, b = int(spans[s, 0]), int(spans[s, 1])
        n = int(rng.integers(1, 6))
        pool[a:min(a + n, b)] = N
        if s and rng.random() < 0.5:
            pool[max(a - 1 - int(rng.integers(0, 3)), 0):a] = N
    for _ in range(15):
        a = int(rng.integers(0, len(pool)))
        pool[a:a + int(rng.integers(2, 9))] = N
    arrs = [_walk(rng, int(rng.choice([1, 2, 17, 60, 100])), 4, S, float(rng.choice([0, 0.1, 0.5, 0.9, 1.0]))) for _ in range(3)]
    w = _walk(rng, int(rng.integers(1, 15)), 4, S, 0.5)
    twin = _walk(rng, int(rng.integers(2, 20)), 4, S, 1.0)
    arrs += [np.concatenate([w, w ^ 1]), np.array([h(5), h(5, True)], np.uint32), twin, twin.copy(), twin[::-1] ^ 1,
             np.array([h(6), h(6, True), h(7, True), h(7, True)], np.uint32)]  # turns into 7+,7+,6+,6-
    for a in arrs:  # x-,x+ is left out: the reference's printer never returns from the link x- -> x+ (gfa.py:196-201)
        for i in np.flatnonzero((a[:-1] & 1 == 1) & (a[1:] == a[:-1] ^ 1)).tolist():
            a[i + 1] = a[i]
    hub = (rng.choice(np.arange(4, S), TOPO_LINEAR + 9, replace=False) << 1) | rng.integers(0, 2, TOPO_LINEAR + 9)
    new = np.zeros(2 * len(hub), np.uint32)
    new[1::2] = hub
    arrs.append(new[::-1] ^ 1)  # turns; its pairs look into the hub's row
    arrs = [arrs[i] for i in rng.permutation(len(arrs)).tolist()]
    step_pool, pspans = _step_pool(rng, arrs, 0, 2 * S)
    pairs = induced(arrs, k, 250_000)
    pairs += pairs[:10] + [(b ^ 1, a ^ 1) for a, b in pairs[10:20]] + [(h(9), h(9)), (h(10), h(10, True)), (h(7), h(7))]
    pairs += [(h(0), int(x)) for x in hub[:TOPO_LINEAR + 1]]
    links = [(a, b, [op(0)] if rng.random() < 0.85 else [op(5)]) for a, b in (pairs[i] for i in rng.permutation(len(pairs)).tolist())]
    names = [b"p%d" % i for i in range(len(pspans))]
    p = assemble(spans, pool, step_pool, pspans, names, links, seg_names=_names(rng, S), header=b"VN:Z:1.0")
    assert len(p.segs) <= 140 and len(p.steps) <= 450
    return p


def gfa_text(p: fo.Pools) -> bytes:
    """H, S, P and L lines of a "text" pools (no path has overlaps)."""
    seq = p.seq_data.tobytes()
    name = p.segs["name"].tolist()
    out = [b"H\t" + p.header.tobytes()] if len(p.header) else []
    out += [b"S\t%d\t%s" % (name[i], seq[int(s["seq_start"]):int(s["seq_end"])]) for i, s in enumerate(p.segs)]
    for i, path in enumerate(p.paths):
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])].tolist()
        out.append(b"P\t%s\t%s\t*" % (p.path_name(i), b",".join(b"%d%s" % (name[x >> 1], b"-" if x & 1 else b"+") for x in st)))
    for r in p.links:
        f, t = int(r["from_"]), int(r["to"])
        out.append(b"L\t%d\t%s\t%d\t%s\t%s" % (name[f >> 1], b"-" if f & 1 else b"+", name[t >> 1], b"-" if t & 1 else b"+",
                                                 pm.alignment(p, int(r["ov_start"]), int(r["ov_end"]))))
    return b"\n".join(out) + b"\n"


# ---- the entry points ----
_MAKERS = {"crush": _crush, "flip": _flip, "flatten": _flatten, "print": _print, "topology": _topology, "text": _text}


def make(seed: int, profile: str) -> fo.Pools:
    return _MAKERS[profile](_rng(seed, profile), seed % 1000)


def extras(seed: int, profile: str) -> dict:
    """flatten: NAME and FLATGFA_FLATTEN_CHUNK_LINES; print: FLATGFA_PRINT_CHUNK_ITEMS.  None: the hook is not set."""
    k = seed % 1000
    rng = np.random.default_rng([seed, 99])
    if profile == "flatten":
        p = make(seed, profile)
        n = len(_bed_lines(p, b""))
        return {"nm": [b"", b"g.og", b"n" * (LONG_NAME + 6)][k % 3], "chunk": [None, n // 2 + 1, max(2, n // 5)][k % 3]}
    if profile == "print":
        n = len(ps.item_sizes(pm.gfa(make(seed, profile))))
        return {"chunk": [None, n // 3 + 1, int(rng.integers(40, 150))][k % 3]}
    return {}


def case_census(seed: int, profile: str) -> Dict[str, int]:
    """The census of one case, with the hooks it runs under."""
    ex = extras(seed, profile)
    kw = {key: ex[key] for key in ("nm", "chunk") if key in ex}
    return census(make(seed, profile), profile, **kw)


def census(p: fo.Pools, profile: str, **kw) -> Dict[str, int]:
    return {"crush": census_crush, "flip": census_flip, "flatten": census_flatten, "print": census_print, "topology": census_topology}[profile](p, **kw)
