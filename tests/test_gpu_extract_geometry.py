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


def with_links(p: fo.Pools, f, t, rng):
    lk = np.zeros(len(f), fo.LINK_DT)
    lk["from_"] = (np.asarray(f, np.uint32) << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    lk["to"] = (np.asarray(t, np.uint32) << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    n_ops = rng.integers(0, 3, len(f))
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
