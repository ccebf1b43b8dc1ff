"""The geometry shapes of tests/chop_shapes.py, without a device: each reaches the edge it is named for, chop_model.chop_fast
agrees with chop_model.chop on it (errors included), and the closed forms of F and G agree with the models."""
import numpy as np
import pytest

import chop_model as cm
import chop_shapes as cs


def check_models(s: cs.Shape):
    for links in (False, True):
        err = s.err_links if links else s.err
        if err is None:
            assert cm.same_pools(cm.chop_fast(s.pools, s.c, links), cm.chop(s.pools, s.c, links)), (s.name, links)
        elif s.host:  # (a step or a link past the segments: the reference panics on seg_map)
            with pytest.raises(IndexError):
                cm.chop(s.pools, s.c, links)
            with pytest.raises(IndexError):
                cm.chop_fast(s.pools, s.c, links)


SMALL = cs.shapes_a(cs.SCAN_SMALL) + cs.shapes_b() + cs.shapes_c() + cs.shapes_d() + cs.shapes_e()


@pytest.mark.parametrize("s", SMALL, ids=lambda s: s.name)
def test_fast_model_equals_model(s):
    check_models(s)


def test_scan_counts():
    for n in cs.SCAN_SMALL:
        a, b, p = cs.a_segs(n), cs.a_steps(n), cs.a_paths(n)
        assert len(a.pools.segs) == n and cs.tiles(a.pools)
        assert len(b.pools.steps) == n and cs.tiles(b.pools)
        assert len(p.pools.paths) == n and not cs.tiles(p.pools)
    assert cs.SCAN_FULL[7] == 1 << 20 and all(n > 256 * 4096 for n in cs.SCAN_FULL[8:])


def test_output_totals():
    m = 3
    for t in (2048 * m - 1, 2048 * m, 2048 * m + 1):
        assert len(cm.chop_fast(cs.b_seg_total(t).pools, cs.C).segs) == t
        for tiling in (True, False):
            s = cs.b_step_total(t, tiling)
            assert cs.tiles(s.pools) == tiling and len(cm.chop_fast(s.pools, cs.C).steps) == t
        s = cs.d_chunk(t)
        assert s.pools.paths["steps_end"] - s.pools.paths["steps_start"] == 256 and not cs.tiles(s.pools)
        assert len(cm.chop_fast(s.pools, cs.C).steps) == t


def source_tiles_per_output_tile(k):
    """For piece counts k, how many 256-element source tiles each 2048-item output tile draws on."""
    first = np.concatenate([[0], np.cumsum(k)])
    out = []
    for j0 in range(0, int(first[-1]), 2048):
        j1 = min(j0 + 2048, int(first[-1]))
        e0 = np.searchsorted(first, j0, side="right") - 1
        e1 = np.searchsorted(first, j1 - 1, side="right") - 1
        out.append(int(e1 // 256 - e0 // 256 + 1))
    return out


def test_nine_source_tiles():
    s = cs.b_nine_tiles(False)
    lens = (s.pools.segs["seq_end"] - s.pools.segs["seq_start"]).astype(np.int64)
    k = np.where(lens <= cs.C, 1, (lens - 1) // cs.C + 1)
    n = source_tiles_per_output_tile(k)
    assert max(n) == 9 and n[1:-1] == [9] * (len(n) - 2)
    s = cs.b_nine_tiles(True)
    lens = (s.pools.segs["seq_end"] - s.pools.segs["seq_start"]).astype(np.int64)
    k = np.where(lens <= cs.C, 1, (lens - 1) // cs.C + 1)[s.pools.steps.astype(np.int64) >> 1]
    n = source_tiles_per_output_tile(k)
    assert max(n) == 9 and n[1:-1] == [9] * (len(n) - 2)


def test_whole_tiles():
    for as_steps in (False, True):
        for lead in (0, 1000):
            q = cm.chop_fast(cs.b_whole_tiles(3, lead, as_steps).pools, cs.C)
            if as_steps:  # the big segment's 6144 pieces, in order or reversed
                d = np.unique(np.diff(q.steps[lead:lead + 6144].astype(np.int64) >> 1))
                assert d.tolist() in ([1], [-1]) and {0, 6143} <= set((q.steps[lead:lead + 6144] >> 1).tolist())
            else:
                assert (q.segs["seq_end"] - q.segs["seq_start"])[lead:lead + 6144].tolist() == [cs.C] * 6144


def test_tile_edge_spans():
    for n_tiles, rem in ((12, 0), (12, 1), (12, 255), (1, 0)):
        p = cs.c_edges(n_tiles, rem).pools
        b, e = p.paths["steps_start"].astype(np.int64), p.paths["steps_end"].astype(np.int64)
        assert cs.tiles(p) and len(p.steps) == 256 * n_tiles + rem
        assert b[0] == e[0] == 0 and b[-1] == e[-1] == len(p.steps)
        if n_tiles > 2:
            assert {255, 256, 257, 511, 512, 513} <= set(b.tolist()) and ((b == 512) & (e == 512)).any()
    assert cs.tiles(cs.c_many_paths(1000).pools) and len(cs.c_many_paths(1000).pools.paths) == 1000


def test_one_trigger_each():
    base = cs.d_trigger("none").pools
    assert cs.tiles(base)

    def triggers(p):
        b, e = p.paths["steps_start"].astype(np.int64), p.paths["steps_end"].astype(np.int64)
        prev = np.concatenate([[0], e[:-1]])
        return int((b != prev).sum()) + int(len(e) > 0 and e[-1] != len(p.steps))

    assert {k: triggers(cs.d_trigger(k).pools) for k in cs.D_TRIGGERS} == {
        "gap_first": 1, "gap_between": 1, "trailing": 1, "swapped": 4, "repeated": 1, "no_paths": 0}
    assert len(cs.d_trigger("no_paths").pools.paths) == 0 and len(cs.d_trigger("no_paths").pools.steps) > 0


def test_errors_where_a_path_walks():
    e = {s.name: s for s in cs.shapes_e()}
    g = e["E_bad_step_in_gap"].pools
    assert (g.steps >> 1).max() >= len(g.segs) and not cs.tiles(g)
    # the model walks the paths only, as chop.rs does
    assert len(cm.chop(g, cs.C).steps) == len(cm.chop_fast(g, cs.C).steps) > 0
    p = e["E_span_past_end"].pools
    assert p.paths["steps_end"].max() > len(p.steps)
    p = e["E_span_reversed"].pools
    assert (p.paths["steps_start"] > p.paths["steps_end"]).any()


@pytest.mark.parametrize("c", cs.F_CS)
def test_u64_lengths_closed_form(c):
    s = cs.f_shape(c)
    first, new_len, steps = cs.f_expect(cs.f_lens(c), c)
    q = cm.chop(s.pools, c)
    assert (q.segs["seq_end"].astype(np.int64) - q.segs["seq_start"].astype(np.int64)).tolist() == new_len
    assert q.steps.tolist() == steps
    assert q.paths["steps_end"].tolist() == [len(steps)]
    if c <= 1 << 40:  # (chop_fast's int64 arithmetic does not hold c = 2^63)
        assert cm.same_pools(cm.chop_fast(s.pools, c), q)
    assert all(0 <= x <= min(c, 2**32 - 1) for x in new_len) and len(new_len) == first[-1]


@pytest.mark.parametrize("c", [1, 7])
@pytest.mark.parametrize("trailing", [False, True])
@pytest.mark.parametrize("n_b", [3, 4])
def test_limit_closed_form_scaled_down(c, trailing, n_b):
    lim = cs.Limit(1000, n_b, c, trailing)
    q = cm.chop_fast(lim.pools(), c)
    assert len(q.segs) == lim.S2 and len(q.steps) == lim.N2
    assert np.array_equal(lim.steps_at(np.arange(lim.N2, dtype=np.int64)), q.steps.astype(np.int64))
    assert np.array_equal(lim.seg_len_at(np.arange(lim.S2, dtype=np.int64)), (q.segs["seq_end"] - q.segs["seq_start"]).astype(np.int64))
    assert cm.seg_first(lim.pools(), c).tolist() == lim.seg_first()
    assert q.paths["steps_start"].tolist() == [0] and q.paths["steps_end"].tolist() == [lim.N2]
    assert cs.tiles(lim.pools()) != trailing


def test_limits():
    for lim in cs.LIMIT_OK:
        assert lim.S2 == 2**31 - 1 and lim.N2 == 2**32 - 1
    for lim in cs.LIMIT_N2:
        assert lim.N2 == 2**32
    # k_expand_paths' one chunk holds all of N' (the u32 loop counter this pins)
    steps, b, e, _, _ = cs.LIMIT_OK[1].arrays()
    assert e[0] - b[0] <= 256 and len(steps) == e[0] + 1
