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


# ---- the shapes aimed at scan, batch and wave seams: they hold the closed form too (above), and they can fail ----

def oracle_group(pools, pid, st, en, m=0):
    """The oracle on one group whose cursor has already seen an interval that ends at m."""
    if not m:
        return fo.interval_depth(pools, pid, st, en)
    return fo.interval_depth(pools, pid, np.concatenate([[0], st]).astype(np.uint64), np.concatenate([[m], en]).astype(np.uint64))[1:]


def long_group_seams():
    s = ish.shape("long_groups")
    return [(label, q) for label, qs in s.seams.items() for q in qs]


@pytest.mark.parametrize("label,seam", long_group_seams(), ids=lambda x: str(x))
def test_long_groups_lose_terms_across_every_seam(label, seam):
    """An M that is not carried across the seam (the group cut there: a scan that drops its carry at a tile, at k_spine's
    second round, at the stride) gives other bytes behind the seam."""
    s = ish.shape("long_groups")
    ids, st, en = s.lists[label]
    assert len(im.runs(ids)) == 1 and 0 < seam < len(ids)
    whole = im.intervals_depth(s.pools, ids, st, en)
    behind = fo.interval_depth(s.pools, int(ids[0]), st[seam:], en[seam:])
    assert (whole[seam:] != behind).any(), (label, seam)
    assert whole[seam] != behind[0], "the seam's own interval"


@pytest.mark.parametrize("head", ish.shape("long_groups").heads["heads"])
def test_long_groups_restart_at_every_head(head):
    """An M that runs on over the head (the two groups merged: a scan that misses a head flag on a tile's first or last
    element) gives other bytes behind the head."""
    s = ish.shape("long_groups")
    ids, st, en = s.lists["heads"]
    groups = im.runs(ids)
    k = [a for a, _ in groups].index(head)
    (a0, b0), (a1, b1) = groups[k - 1], groups[k]
    assert b0 == a1 == head
    want = im.intervals_depth(s.pools, ids, st, en)[a1:b1]
    merged = oracle_group(s.pools, int(ids[a1]), st[a1:b1], en[a1:b1], m=int(en[a0:b0].max()))
    assert (want != merged).any() and want[0] != merged[0], head


def test_long_groups_are_mostly_not_zero():
    s = ish.shape("long_groups")
    assert sorted(s.lists) == ["heads", "spine_round", "stride", "through_a_tile", "tile_seams"]
    for label, (ids, st, en) in s.lists.items():
        out = im.intervals_depth(s.pools, ids, st, en)
        assert 2 * np.count_nonzero(out) >= len(out), (label, np.count_nonzero(out), len(out))
    assert [len(s.lists[x][0]) for x in ("tile_seams", "spine_round", "stride")] == [3 * 1024 + 5, 262144 + 1024 + 3, 524288 + 257]


def test_many_paths_and_cut_edges_cover_what_they_say():
    s = ish.shape("many_paths")
    order, counts = s.notes["order"], s.notes["counts"]
    ids = s.lists["slot_order"][0]
    groups = [int(ids[a]) for a, _ in im.runs(ids)]
    assert groups == [int(p) for p in order], "the list names every path once, in slot order"
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in s.pools.paths]
    assert [lengths[p] for p in groups] == [int(c) for c in counts]
    for name in s.lists:
        i = s.lists[name][0]
        g = [int(i[a]) for a, _ in im.runs(i)]
        for budget in (1, 1024, 2048, 1 << 27):
            assert len(ish.plan_slots(g, lengths, budget)) == ish.plan_batches(g, lengths, budget), (name, budget)
    at = s.notes["at_tile"]
    run = [int(p) for p in order[at:at + 3]]
    # budget 1, around the runs: each run of stepless paths is a batch of its own, of no steps
    i = s.lists["around_the_runs"][0]
    g = [int(i[a]) for a, _ in im.runs(i)]
    plan = ish.plan_slots(g, lengths, 1)
    for r in ([int(p) for p in order[:3]], run, [int(order[s.notes["at_two"]])], [int(p) for p in order[-3:]]):
        assert r in plan, "a run of stepless paths is not cut at both ends"
    # budget 1024, the whole list: the first batch is 1024 steps and ends in the run
    plan = ish.plan_slots(groups, lengths, 1024)
    assert plan[0][-3:] == run and sum(lengths[p] for p in plan[0]) == 1024 and lengths[plan[1][0]] > 0
    assert {label: batches for label, _, _, batches in ish.run_budget_cases()} == {"runs-budget1": 33, "budget1024": 8, "budget2048": 7}
    c = ish.shape("cut_edges")
    assert len(c.lists) == 18 + 8
    assert (c.pools.seg_lens() == 0).any()


def fused_window_table(pools, window, path_ids) -> bytes:
    """The window table as one job over runs of equal ids made it: a path listed again behind itself, or behind paths without
    windows, goes on in the group of its first listing."""
    lens, _ = fo.path_depth(pools)
    rows, ids = [], []
    for p in path_ids:
        for a, b in im.windows(int(lens[p]), window):
            rows.append((pools.path_name(p), a, b))
            ids.append(p)
    return fo._emit_intervals(rows, im.intervals_depth(pools, ids, [r[1] for r in rows], [r[2] for r in rows]))


@pytest.mark.parametrize("paths,size,lines", [([0, 0], 932, 27), ([0, 2, 0], 932, 27), ([1, 1, 3], 815, 18)], ids=str)
def test_a_repeated_path_is_not_one_group(paths, size, lines):
    """What flatgfa_window_depth_paths_table promises is the per-path join; the fused groups give other bytes."""
    pools = ish.shape("basic").pools
    want = im.window_depth_paths_table(pools, 50, paths)
    fused = fused_window_table(pools, 50, paths)
    assert len(want) == size and len(want.splitlines()) == len(fused.splitlines())
    assert sum(1 for a, b in zip(want.splitlines(), fused.splitlines()) if a != b) == lines


def test_big_products_round():
    """The case the GPU test builds from raw arrays: some product depth * len and some end - start is no f64, and the
    closed form, in Python integers with a correctly rounded float(), is what the expected bytes come from."""
    pools, depth, ids, st, en = ish.big_products()
    lens = pools.seg_lens().astype(np.uint64)
    assert int(lens.max()) == int(depth.max()) == 2 ** 32 - 1
    prods = [int(d) * int(n) for d, n in zip(depth, lens)]
    assert any(p > 2 ** 53 and int(float(p)) != p for p in prods)
    widths = [int(b) - int(a) for a, b in zip(st, en) if b > a]
    assert any(w > 2 ** 53 and int(float(w)) != w for w in widths)
    assert (0, 2 ** 64 - 1) in zip(st.tolist(), en.tolist()) and (1, 2 ** 63 + 1) in zip(st.tolist(), en.tolist())
    out = im.closed_form(pools, ids, st, en, depth)
    assert np.count_nonzero(out) > len(out) // 4 and np.isfinite(out).all()
