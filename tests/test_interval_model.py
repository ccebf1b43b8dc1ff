"""The closed form the interval kernels implement (tests/interval_model.py: closed_form) against the reference's loop
(intervals_depth: the oracle's interval_depth, group by group), bytewise, on every shape of tests/interval_shapes.py and on
seeded random lists -- before any GPU run.  No GPU."""
import numpy as np
import pytest

import interval_model as im
import interval_shapes as ish
from oracle import flatgfa_oracle as fo


@pytest.mark.parametrize("name", [f.__name__ for f in ish.SHAPES])
def test_closed_form_on_shapes(name):
    s = ish.shape(name)
    depth = fo.seg_depth(s.pools)
    assert s.lists
    for label, (ids, st, en) in s.lists.items():
        want = im.intervals_depth(s.pools, ids, st, en)
        got = im.closed_form(s.pools, ids, st, en, depth)
        assert got.tobytes() == want.tobytes(), (name, label, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("seed", range(4))
def test_closed_form_on_random_lists(seed):
    """A thousand lists a seed: unsorted, overlapping, inverted, past the end, over steps of no length."""
    rng = np.random.default_rng(100 + seed)
    S = 12
    lens = rng.integers(0, 6, S)
    steps = ((rng.integers(0, S, 80) << 1) | rng.integers(0, 2, 80)).astype(np.uint32)
    pools = ish.make_pools(lens, steps, [(0, 30), (20, 70), (70, 70), (75, 80)])
    depth = fo.seg_depth(pools)
    top = max((ish.ends_of(pools, p) or [0])[-1] for p in range(4)) + 4
    for _ in range(1000):
        n = int(rng.integers(1, 9))
        ids = rng.integers(0, 4, n) if rng.integers(0, 2) else np.full(n, rng.integers(0, 4))
        st = rng.integers(0, top, n)
        en = np.maximum(st + rng.integers(-2, top, n), 0)
        want = im.intervals_depth(pools, ids, st, en)
        got = im.closed_form(pools, ids, st, en, depth)
        assert got.tobytes() == want.tobytes(), (seed, ids, st, en, got, want)


def test_shapes_cover_what_they_say():
    b = ish.shape("basic")
    spans = [(int(p["steps_start"]), int(p["steps_end"])) for p in b.pools.paths]
    assert spans[1][0] < spans[0][1] and spans[3][0] > spans[2][1] and spans[2][0] == spans[2][1]  # overlap, gap, no steps
    assert (b.pools.seg_lens() == 0).any()
    ids, st, en = b.lists["aba"]
    assert im.runs(ids) == [(0, 1), (1, 2), (2, 3)]
    ids, st, en = ish.shape("many_groups").lists["alternating"]
    assert len(im.runs(ids)) == len(ids) > ish.LONG_WAVES
    t = ish.shape("tiles")
    counts = sorted(int(p["steps_end"]) - int(p["steps_start"]) for p in t.pools.paths)
    assert counts == [ish.TILE - 1, ish.TILE, ish.TILE + 1, 2 * ish.TILE - 1, 2 * ish.TILE, 2 * ish.TILE + 1]
    lp = ish.shape("long_positions")
    assert all(ish.ends_of(lp.pools, p)[-1] > 1 << 32 for p in range(2))
    # an interval where M drops terms: the nested list's results differ from the same intervals taken one group each
    ids, st, en = b.lists["p0_nested"]
    together = im.intervals_depth(b.pools, ids, st, en)
    alone = np.concatenate([im.intervals_depth(b.pools, ids[k:k + 1], st[k:k + 1], en[k:k + 1]) for k in range(len(ids))])
    assert (together != alone).any()


def test_budget_cases_cut_where_they_say():
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in ish.shape("basic").pools.paths]
    assert lengths == [300, 200, 0, 130]
    for label, groups, budget, batches in ish.budget_cases():
        assert ish.plan_batches(groups, lengths, budget) == batches, label


def test_tables_of_the_model():
    p = fo.parse_gfa(b"S\t1\tACGT\nS\t2\tAC\nP\tx\t1+,2+\t*\nP\ty\t2+\t*\n")
    assert im.window_depth_paths_table(p, 4) == fo.window_depth_table(p, b"x", 4) + fo.window_depth_table(p, b"y", 4)
    bed = b"y\t0\t2\nx\t0\t6\nx\t1\t3\ny\t1\t2\n"
    assert im.bed_depth_paths_table(p, bed) == b"y\t0\t2\t2\nx\t0\t6\t1.3333\nx\t1\t3\t0\ny\t1\t2\t2\n"  # ([1, 3) behind [0, 6): the cursor is past it)
