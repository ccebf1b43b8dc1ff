"""extract and position on graphs large enough to take every kernel over its tile, grid and 32-bit edges, against the numpy
form of the model (tests/extract_model.py: extract_fast, pinned to the sequential form on the CPU).  Run with -m gpu."""
import os

import numpy as np
import pytest

import chop_model as cm
import extract_model as em
import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from test_gpu_extract import extract_id, load_pools, same

pytestmark = pytest.mark.gpu


def with_links(p: fo.Pools, f, t, rng, n_ops=None):
    """p with the links f[i] -> t[i], random orientations, and n_ops[i] (0 .. 2 where not given) alignment ops each."""
    lk = np.zeros(len(f), fo.LINK_DT)
    lk["from_"] = (np.asarray(f, np.uint32) << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    lk["to"] = (np.asarray(t, np.uint32) << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    n_ops = rng.integers(0, 3, len(f)) if n_ops is None else n_ops
    off = np.concatenate([[0], np.cumsum(n_ops)])
    lk["ov_start"], lk["ov_end"] = off[:-1], off[1:]
    q = fo.Pools(**{n: getattr(p, n) for n in fo.POOL_ORDER})
    q.links = lk
    q.alignment = ((rng.integers(1, 200, int(off[-1])) << 8) | rng.integers(0, 4, int(off[-1]))).astype(np.uint32)
    return q


def check(p, cases):
    g, path = load_pools(p)
    try:
        out = []
        for origin, c, d, e in cases:
            want = em.extract_fast(p, origin, c, d, e)
            q = extract_id(g, origin, c, d, e)
            same(q, want, (origin, c, d, e))
            out.append((q, want))
        return out
    finally:
        g.close()
        os.unlink(path)


def test_links_past_one_grid_and_the_whole_graph():
    # 700 000 links: k_bfs_level's grid of 2048 workgroups goes round twice; at c = 64 the neighbourhood is the whole graph
    rng = np.random.default_rng(1)
    S = 200_000
    p = cm.pools_of(pa.synth(3, S, 12, 100_000, "pangenome", True))
    f = np.concatenate([np.arange(S - 1), rng.integers(0, S, 500_001)])
    t = np.concatenate([np.arange(1, S), rng.integers(0, S, 500_001)])
    p = with_links(p, f, t, rng)
    res = check(p, [(5, 1, 300000, 6), (5, 3, 100, 1), (S - 1, 64, 0, 0)])
    q, want = res[-1]
    assert len(want.segs) == S and len(want.links) == len(p.links) and len(want.steps) == len(p.steps)
    # extract, then depth and chop on the result
    d, u = q.seg_depth_with_uniq()
    wd, wu = fo.seg_depth_with_uniq(want)
    assert np.array_equal(d, wd) and np.array_equal(u, wu)
    q2, want2 = res[1]
    assert cm.same_pools(cm.pools_of(q2.chop(3, True)), cm.chop_fast(want2, 3, True))


def planted(rng, n_segs, member, path_lens, lens=None):
    """Segments 0 .. n_segs; step i walks a member segment (1 .. 9, linked to the origin 0) iff member[i]."""
    lens = rng.integers(1, 9, n_segs).astype(np.int64) if lens is None else lens
    st = np.concatenate([[0], np.cumsum(lens)[:-1]])
    segs = np.zeros(n_segs, fo.SEG_DT)
    segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, n_segs + 1), st, st + lens
    n = len(member)
    seg = np.where(member, rng.integers(0, 10, n), rng.integers(10, n_segs, n)).astype(np.uint32)
    steps = (seg << 1) | rng.integers(0, 2, n).astype(np.uint32)
    paths = np.zeros(len(path_lens), fo.PATH_DT)
    ends = np.cumsum(path_lens)
    assert ends[-1] == n
    names = b"".join(b"p%d" % k for k in range(len(path_lens)))
    ne = np.cumsum([len(b"p%d" % k) for k in range(len(path_lens))])
    paths["name_start"], paths["name_end"] = ne - [len(b"p%d" % k) for k in range(len(path_lens))], ne
    paths["steps_start"], paths["steps_end"] = ends - path_lens, ends
    z = np.zeros(0, np.uint8)
    p = fo.Pools(header=np.frombuffer(b"VN:Z:1.0", np.uint8).copy(), segs=segs, paths=paths, links=np.zeros(0, fo.LINK_DT), steps=steps,
                 seq_data=rng.choice(np.frombuffer(b"ACGT", np.uint8), int(lens.sum())), overlaps=np.zeros(0, fo.SPAN_DT),
                 alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(names, np.uint8).copy(), optional_data=z, line_order=z)
    return with_links(p, np.zeros(9, np.int64), np.arange(1, 10), rng)


def test_one_path_over_many_tiles_thousands_in_one_and_runs_on_tile_edges():
    rng = np.random.default_rng(2)
    # a path of 1 500 000 steps (1 465 scan tiles), then 6 000 paths of 0 .. 3 steps (hundreds of them, empty ones among them,
    # in one tile), then one of 300 000
    small = rng.integers(0, 4, 6000)
    path_lens = np.concatenate([[1_500_000], small, [300_000]]).astype(np.int64)
    n = int(path_lens.sum())
    i = np.arange(n)
    member = (i // 1024) % 3 == 0          # runs that start and end exactly on tile edges
    member |= (i % 4096 == 1023) | (i % 4096 == 2049)  # ... one step before and one after an edge
    member[1_500_000:1_500_000 + int(small.sum())] = rng.random(int(small.sum())) < 0.5
    member[-1] = True                      # a run that ends with the pool
    p = planted(rng, 5000, member, path_lens)
    check(p, [(0, 1, 0, 0), (0, 1, 40, 2), (0, 0, 300000, 1)])


def test_positions_past_32_bits_and_megabase_gathers():
    # four segments that share one sequence span of 2^20 bases; a path of 6 000 steps is 6.3e9 bases long
    rng = np.random.default_rng(4)
    n = 6000
    member = rng.random(n) < 0.3
    member[-1] = True
    p = planted(rng, 16, member, np.array([n], np.int64), lens=np.full(16, 1 << 20, np.int64))
    p.segs["seq_start"], p.segs["seq_end"] = 0, 1 << 20
    p.seq_data = p.seq_data[:1 << 20].copy()
    (q, want), = check(p, [(0, 1, 0, 0)])
    ends = [int(want.path_name(k).rsplit(b"-", 1)[1]) for k in range(len(want.paths))]
    assert max(ends) == n << 20 and max(ends) > 1 << 32 and len(want.seq_data) == 10 << 20
    g, path = load_pools(p)
    try:
        seg = p.steps >> 1
        for off in (0, (1 << 32) - 1, 1 << 32, (1 << 32) + 12345, (n << 20) - 1, n << 20, 1 << 63):
            hit = g.position(b"p0", off)
            if off >= n << 20:
                assert hit is None
            else:
                k = off >> 20
                assert hit == (int(seg[k]) + 1, off & ((1 << 20) - 1), int(p.steps[k]) & 1 == 0), off
    finally:
        g.close()
        os.unlink(path)


def test_position_on_a_path_past_one_grid():
    # 700 000 steps: k_find_pos's grid goes round twice, the scan takes 684 tiles
    g = pa.synth(9, 50_000, 3, 700_000, "pangenome", True)
    p = cm.pools_of(g)
    lens = p.seg_lens().astype(np.int64)
    for pid in (0, 2):
        st = p.steps[int(p.paths[pid]["steps_start"]):int(p.paths[pid]["steps_end"])]
        ends = np.cumsum(lens[st >> 1])
        total = int(ends[-1])
        for off in (0, total // 3, int(ends[1023]) - 1, int(ends[1023]), int(ends[524_288]), total - 1, total):
            k = int(np.searchsorted(ends, off, side="right"))
            want = None if k == len(st) else (int(p.segs[st[k] >> 1]["name"]), off - (int(ends[k - 1]) if k else 0), int(st[k]) & 1 == 0)
            assert g.position(p.path_name(pid), off) == want, (pid, off)


def test_heads_and_kept_links_planted_on_tile_and_spine_round_edges():
    # the scan's tile is 1 024 elements and its spine goes round every 256 tiles: paths start exactly at steps 1 024, 2 048,
    # 262 144 (the first step behind a round) and 262 145, with member steps on both sides of every start; the links kept
    # at 1 023, 1 024, 262 143 and 262 144 carry alignment ops and the links next to them none
    rng = np.random.default_rng(6)
    path_lens = np.array([1024, 1024, 260_096, 1, 2500], np.int64)
    starts = np.cumsum(path_lens)[:-1]
    assert list(starts) == [1024, 2048, 262_144, 262_145]
    n = int(path_lens.sum())
    member = rng.random(n) < 0.4
    for s in starts:
        member[s - 1:s + 2] = True
    p = planted(rng, 3000, member, path_lens)
    L = 262_144 + 1700
    kept = rng.random(L) < 0.05
    edges = np.array([1023, 1024, 262_143, 262_144])
    kept[edges] = True
    kept[[1022, 262_145]], kept[[1025, 262_142]] = True, False
    f = np.where(kept, rng.integers(1, 10, L), rng.integers(10, 3000, L))
    t = np.where(kept, rng.integers(1, 10, L), rng.integers(10, 3000, L))
    f[:9], t[:9] = 0, np.arange(1, 10)  # (what makes 1 .. 9 the origin's neighbours)
    n_ops = rng.integers(0, 3, L)
    n_ops[edges] = [1, 2, 2, 1]
    n_ops[[1022, 1025, 262_142, 262_145]] = 0
    p = with_links(p, f, t, rng, n_ops)
    res = check(p, [(0, 1, 0, 0), (0, 1, 40, 2)])
    want = res[0][1]
    assert len(want.segs) == 10 and len(want.steps) == int(member.sum())
    # every planted start opens a subpath at position 0 of its path, and the step before it closes one
    names = [want.path_name(k) for k in range(len(want.paths))]
    for k in range(1, 5):
        assert sum(nm.startswith(b"p%d:0-" % k) for nm in names) == 1
    assert len(want.links) == int(kept[9:].sum()) + 9 and len(want.alignment) == int(n_ops[9:][kept[9:]].sum() + n_ops[:9].sum())


def shared_span_graph(n_segs, n_links, self_loops):
    """n_segs segments that share one sequence span of 2^20 bases, chained by links; or one segment with n_links self-loops
    that all carry the whole alignment pool of 2^20 ops.  (Spans may overlap: the loader wants each inside its pool.)"""
    rng = np.random.default_rng(8)
    big = 1 << 20
    segs = np.zeros(n_segs, fo.SEG_DT)
    segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, n_segs + 1), 0, (4 if self_loops else big)
    lk = np.zeros(n_links, fo.LINK_DT)
    if self_loops:
        lk["from_"], lk["to"], lk["ov_start"], lk["ov_end"] = 0, rng.integers(0, 2, n_links), 0, big
        align = ((rng.integers(1, 200, big) << 8) | rng.integers(0, 4, big)).astype(np.uint32)
    else:
        lk["from_"], lk["to"] = np.arange(n_links) << 1, (np.arange(1, n_links + 1) << 1) | rng.integers(0, 2, n_links)
        align = np.zeros(0, np.uint32)
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=np.frombuffer(b"VN:Z:1.0", np.uint8).copy(), segs=segs, paths=np.zeros(0, fo.PATH_DT), links=lk,
                    steps=np.zeros(0, np.uint32), seq_data=rng.choice(np.frombuffer(b"ACGT", np.uint8), 4 if self_loops else big),
                    overlaps=np.zeros(0, fo.SPAN_DT), alignment=align, name_data=z, optional_data=z, line_order=z)


def refused(p, origin, c):
    g, path = load_pools(p)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            extract_id(g, origin, c, 0, 0)
        return e.value
    finally:
        g.close()
        os.unlink(path)


def test_alignment_ops_reaching_32_bits_are_refused():
    # 4 096 self-loops (kept at c = 0: both ends are the origin) times 2^20 ops is 2^32 exactly: a 32-bit total reads 0
    e = refused(shared_span_graph(1, 4096, True), 0, 0)
    assert e.code == -6 and "would hold 4294967296 alignment ops" in str(e)
    # ... and eight of them make a subgraph of 2^23 ops
    (q, want), = check(shared_span_graph(1, 8, True), [(0, 0, 0, 0)])
    assert len(want.links) == 8 and len(want.alignment) == 8 << 20 and int(want.links["ov_end"][-1]) == 8 << 20


def test_sequences_reaching_32_bits_are_refused():
    # 4 097 segments of 2^20 bases: the 4 096th takes the subgraph's sequences to 2^32
    e = refused(shared_span_graph(4097, 4096, False), 2048, 4097)
    assert e.code == -6 and "sequences or optional data pass 2^32 - 1 bytes" in str(e)
    (q, want), = check(shared_span_graph(8, 7, False), [(4, 8, 0, 0)])
    assert len(want.segs) == 8 and len(want.seq_data) == 8 << 20
