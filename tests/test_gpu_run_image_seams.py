"""The run-length image of the steps where tests/test_gpu_run_image.py does not look: one image read
by plans whose graphs differ, every window width the rule admits, the control ring of k_scan_runs used more than once, its
non-temporal builds, calls issued while the image is pending, plans closed and told `steps_changed` in every order, the rule's
refusals that guard a wrong answer, and the ends of the step array.

Every expected vector is the C oracle's on the same pools, compared bit for bit.  A test that expects the image asserts that
the description names it: the calls behind `describe()` then ran k_scan_runs, not k_scan.  The description also says what the
image was made of (`run_image_steps`), how many plans hold it (`run_image_plans`) and how it is read (`run_image_reads`).

Not covered: the BIG builds of k_scan_runs (bucket arrays of 2^30 records and more) cannot be reached at test sizes.
"""
import dataclasses
import re

import numpy as np
import pytest

import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from oracle import synth
from test_gpu_run_image import IMAGE, OFF, answers, check, env, laid_out, make_pools, spans_of  # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu

STEPS_OF = re.compile(r" run_image_steps=(\d+)\b")
PLANS_OF = re.compile(r" run_image_plans=(\d+)\b")
READS = re.compile(r" run_image_reads=(\w+)")


def off_reason(desc):
    assert OFF.search(desc), desc
    return OFF.search(desc).group(1)


def same(got, want, uniq=True):
    return bool((got[0] == want[0]).all()) and (not uniq or bool((got[1] == want[1]).all()))


# ---- A. one image, graphs that differ ----

def shared_graphs(steps, specs):
    """One int32 step tensor on the device, wrapped once per (begins, ends, n_segs, n_steps) of `specs` (n_steps: the graph
    is over the first n_steps of the tensor): the graphs share the steps' address.  Returns [(graph, pools)]."""
    import torch
    from pollen_amd.device import DeviceGraph
    steps = np.ascontiguousarray(steps, dtype=np.uint32)
    buf = torch.from_numpy(steps.view(np.int32)).to("cuda:0")
    out = []
    for begins, ends, n_segs, n_steps in specs:
        b = np.ascontiguousarray(begins, dtype=np.uint32)
        e = np.ascontiguousarray(ends, dtype=np.uint32)
        part = buf[:n_steps]
        assert part.data_ptr() == buf.data_ptr()
        graph = DeviceGraph.from_tensors(part, torch.from_numpy(b.view(np.int32)).to("cuda:0"), torch.from_numpy(e.view(np.int32)).to("cuda:0"),
                                         n_segs, h_path_begin=b, h_path_end=e)
        out.append((graph, make_pools(steps[:n_steps], b, e, n_segs)))
    torch.cuda.synchronize()
    return out


def two_plans_in_order(graphs, first):
    """A plan per graph; the plan of graphs[first] makes its first call first (the image is made behind that call, with that
    graph's cuts), is asked for its description, then the other one does the same.  Returns [(plan, first answer, description)]
    in the order of `graphs`."""
    from pollen_amd.device import DepthPlan
    plans = [DepthPlan(g) for g, _ in graphs]
    res = [None, None]
    for k in (first, 1 - first):
        got = answers(plans[k], graphs[k][0].n_segs)
        res[k] = (plans[k], got, plans[k].describe())
    return res


def check_shared(graphs, first, one_image):
    res = two_plans_in_order(graphs, first)
    try:
        for k, (plan, got, desc) in enumerate(res):
            graph, pools = graphs[k]
            want = fo.seg_depth_with_uniq(pools)
            assert IMAGE.search(desc), desc
            assert int(STEPS_OF.search(desc).group(1)) == graph.n_steps, desc
            for c, g in enumerate([got] + [answers(plan, graph.n_segs) for _ in range(3)]):
                assert (g[0] == want[0]).all(), (k, c, desc, np.flatnonzero(g[0] != want[0])[:8])
                assert (g[1] == want[1]).all(), (k, c, desc, np.flatnonzero(g[1] != want[1])[:8])
        descs = [r[0].describe() for r in res]
        if one_image:
            assert IMAGE.search(descs[0]).group(1) == IMAGE.search(descs[1]).group(1), descs
            assert [PLANS_OF.search(d).group(1) for d in descs] == ["2", "2"], descs
        else:
            assert [PLANS_OF.search(d).group(1) for d in descs] == ["1", "1"], descs
    finally:
        for plan, _, _ in res:
            plan.close()


def spans_inside_runs():
    """40 spans of a 16 384-step array whose begins and ends fall at 1024k - 1, 1024k, 1024k + 1 and in the middle of blocks;
    most touch (end[i] == begin[i + 1]: at 500 and 1500 in the middle of a run), three leave two steps to nobody, and neither
    the first three steps nor the last two belong to a path."""
    edges = sorted({3, 16_382, 500, 1500, 8192 + 300} | {1024 * k + d for k in range(1, 13) for d in (-1, 0, 1)})
    begins, ends = list(edges[:-1]), list(edges[1:])
    long_ = [i for i in range(len(begins)) if ends[i] - begins[i] > 3]
    for i in (long_[2], long_[6], long_[10]):
        ends[i] -= 2
    assert len(begins) == 40
    return begins, ends


@pytest.mark.parametrize("first", [0, 1], ids=["one_first", "many_first"])
def test_cuts_from_another_graph(env, first):
    # ids 0..8191 up, then 8191..0 down: runs of 1024 steps everywhere, which the one-path graph's image cuts at the block
    # edges only -- every span of the other graph then begins and ends inside an entry and is right by the clip alone
    ids = np.concatenate([np.arange(8192), np.arange(8191, -1, -1)]).astype(np.uint32)
    b, e = spans_inside_runs()
    graphs = shared_graphs(ids << 1, [([0], [16_384], 9_000, 16_384), (b, e, 9_000, 16_384)])
    check_shared(graphs, first, one_image=True)


@pytest.mark.parametrize("first", [0, 1], ids=["all_first", "subset_first"])
def test_a_subset_of_the_paths_reads_the_image_of_all(env, first):
    # the spans flatgfa_seg_depth_subset makes: every third path of a graph, on the graph's own step array
    pools = synth.pools(41, 9_000, 30, 4_000, "pangenome")
    b, e = spans_of(pools)
    graphs = shared_graphs(pools.steps, [(b, e, 9_000, len(pools.steps)), (b[::3], e[::3], 9_000, len(pools.steps))])
    check_shared(graphs, first, one_image=True)


@pytest.mark.parametrize("first", [0, 1], ids=["short_first", "long_first"])
def test_graphs_over_a_shorter_and_a_longer_slice_get_images_of_their_own(env, first):
    # same address, 10 000 and 40 000 steps: the shorter graph's image has an index of 11 words and closes its last run at
    # step 10 000 -- the longer graph's items must not read it (they did, past its end, before n_steps was part of the key)
    pools = synth.pools(43, 9_000, 4, 10_000, "pangenome")
    b, e = spans_of(pools)
    assert int(e[-1]) == 40_000
    graphs = shared_graphs(pools.steps, [([0, 6_000], [6_000, 10_000], 9_000, 10_000), (b, e, 9_000, 40_000)])
    check_shared(graphs, first, one_image=False)


@pytest.mark.parametrize("first", [0, 1], ids=["small_first", "large_first"])
def test_an_id_is_checked_against_the_readers_own_n_segs(env, first):
    pools = synth.pools(47, 12_000, 6, 8_000, "pangenome")
    assert int((pools.steps >> 1).max()) >= 9_000
    b, e = spans_of(pools)
    n = len(pools.steps)
    graphs = shared_graphs(pools.steps, [(b, e, 9_000, n), (b, e, 12_000, n)])
    from pollen_amd.device import DepthPlan
    plans = [DepthPlan(g) for g, _ in graphs]
    want = fo.seg_depth_with_uniq(graphs[1][1])

    def call(k):
        if k == 1:
            got = answers(plans[1], 12_000)
            assert same(got, want), k
        else:
            with pytest.raises(pa.FlatGFAError) as err:
                answers(plans[0], 9_000)
            assert err.value.code == -2

    try:
        for k in (first, 1 - first):
            call(k)
            assert IMAGE.search(plans[k].describe()), plans[k].describe()
        for _ in range(3):
            call(0)
            call(1)
        descs = [p.describe() for p in plans]
        assert [PLANS_OF.search(d).group(1) for d in descs] == ["2", "2"], descs
    finally:
        for p in plans:
            p.close()


# ---- B. window widths ----

def runs_at_window_offsets(wb):
    """16 384 segments; runs of exactly 1024 steps, each on an aligned block of the step array, whose lowest id sits at window
    offset 0, 1, W - 1024, W - 1023, W - 1 and W - 512: the longest record that does not cross an edge, first parts of 1, 1023
    and 512, and the run that ends exactly on the edge.  One path walks them upwards, a second one downwards."""
    W = 1 << wb
    n_win = 16_384 // W
    ups, downs = [], []
    for k, off in enumerate([0, 1, W - 1024, W - 1023, W - 1, W - 512]):
        low = (k % (n_win - 1)) * W + off
        assert low + 1023 < 16_384
        ups.append(np.arange(low, low + 1024))
        downs.append(np.arange(low + 1023, low - 1, -1))
    # (the second path walks the first run once more behind the others: a revisit, so unique depth differs from depth)
    steps, b, e = laid_out([np.concatenate(ups), np.concatenate(downs + ups[:1])])
    assert b[1] % 1024 == 0
    return make_pools(steps, b, e, 16_384)


def zigzag_pools():
    a = np.tile([5, 6], 1500)
    b_ = np.tile([10, 11, 12, 11], 700)
    c = np.tile([20, 21, 22, 21, 20, 19], 500)
    steps, b, e = laid_out([a, b_, c], lead=3)
    return make_pools(steps, b, e, 9_000)


def split_pools():
    paths = [np.arange(10, 8010), np.arange(8500, 500, -1), np.concatenate([np.arange(0, 3000), np.arange(2000, 5000)])]
    steps, b, e = laid_out(paths, lead=7)
    return make_pools(steps, b, e, 9_000)


def windows_of(desc):
    return re.search(r" windows=(\d+)x(\d+)", desc).groups()


@pytest.mark.parametrize("wb,mall", [(11, None), (12, None), (12, "0"), (13, None)], ids=["11", "12", "12_nt", "13"])
def test_runs_of_1024_at_every_window_offset(env, wb, mall):
    env.setenv("FLATGFA_WB", str(wb))
    if mall is not None:
        env.setenv("FLATGFA_MALL_MB", mall)
    pools = runs_at_window_offsets(wb)
    want = fo.seg_depth_with_uniq(pools)
    assert (want[0] != want[1]).any()
    desc = check(env, pools, want=want)
    assert windows_of(desc) == (str(16_384 >> wb), str(1 << wb)), desc
    assert READS.search(desc).group(1) == ("nt" if mall == "0" else "plain"), desc


@pytest.mark.parametrize("case", ["zigzag", "split", "pangenome"])
@pytest.mark.parametrize("wb", [11, 13])
def test_the_other_widths_on_the_shapes_of_the_default_one(env, wb, case):
    env.setenv("FLATGFA_WB", str(wb))
    if case == "split":
        env.setenv("FLATGFA_PIECE_STEPS", "700")
        env.setenv("FLATGFA_ACC_PARTS", "1")
    pools = {"zigzag": zigzag_pools, "split": split_pools}[case]() if case != "pangenome" else synth.pools(7, 9_000, 30, 20_000, "pangenome")
    # pass 2 has no bitsets for split paths with 8192-segment windows: such a plan is not tagged, and keeps k_scan
    image = not (case == "split" and wb == 13)
    desc = check(env, pools, expect_image=image)
    assert windows_of(desc)[1] == str(1 << wb), desc
    if case == "split":
        assert int(re.search(r"split_paths=(\d+)", desc).group(1)) > 0, desc
    if not image:
        assert off_reason(desc) == "untagged", desc


@pytest.mark.parametrize("asked", ["10", "14", "0"])
def test_no_plan_gets_a_width_pass_2_has_no_build_for(env, asked):
    # FLATGFA_WB outside 11..13 is not a width: the plan keeps the one it would have had (4096-segment windows at this size),
    # so `run_image=off(windows)` cannot be reached -- and the 13-bit pass 2 never reads narrower records
    env.setenv("FLATGFA_WB", asked)
    desc = check(env, runs_at_window_offsets(12))
    assert windows_of(desc) == ("4", "4096"), desc


# ---- C. the control ring, one long item, the non-temporal builds ----

@pytest.mark.parametrize("mall", [None, "0"], ids=["plain", "nt"])
def test_every_cell_of_the_control_ring_is_used_again(env, mall):
    # 560 items on 8 workgroups: 70 each, so every one of the 32 cells of the chunk and arrival counters is used twice and
    # six of them three times -- a cell the last wave did not reset hands the next item's waves no chunk at all
    env.setenv("FLATGFA_SCAN_WGS", "8")
    if mall is not None:
        env.setenv("FLATGFA_MALL_MB", mall)
    pools = synth.pools(53, 9_000, 560, 400, "pangenome")
    desc = check(env, pools)
    assert " scan_workgroups=8 " in desc and " items=560 " in desc, desc
    assert READS.search(desc).group(1) == ("nt" if mall == "0" else "plain"), desc


@pytest.mark.parametrize("mall", [None, "0"], ids=["plain", "nt"])
def test_one_item_of_hundreds_of_chunks_beside_short_ones(env, mall):
    # eight paths of 300 steps and one of 200 000 with runs of three (66 667 entries: 261 chunks of 256 off one counter, taken
    # by one workgroup's waves while the other workgroups are long done)
    env.setenv("FLATGFA_SCAN_WGS", "8")
    env.setenv("FLATGFA_PIECE_STEPS", str(1 << 20))  # (the long path stays one item)
    if mall is not None:
        env.setenv("FLATGFA_MALL_MB", mall)
    n_segs = 9_000
    starts = (synth.mix64(np.arange(200_001 // 3, dtype=np.uint64) * synth.GOLDEN) % np.uint64(n_segs - 3)).astype(np.uint32)
    long_ = (starts[:, None] + np.arange(3, dtype=np.uint32)[None, :]).reshape(-1)
    short = synth.pools(59, n_segs, 8, 300, "pangenome").steps >> 1
    steps, b, e = laid_out([short[300 * k:300 * k + 300] for k in range(4)] + [long_] + [short[300 * k:300 * k + 300] for k in range(4, 8)])
    desc = check(env, make_pools(steps, b, e, n_segs))
    assert " scan_workgroups=8 " in desc and " items=9 " in desc and " split_paths=0 " in desc, desc
    assert READS.search(desc).group(1) == ("nt" if mall == "0" else "plain"), desc


# ---- D. call order and lifetime ----

def graph_of(pools):
    from pollen_amd.device import DeviceGraph
    b, e = spans_of(pools)
    return DeviceGraph(pools.steps, b, e, len(pools.segs))


def used_mb():
    import torch
    torch.cuda.synchronize()
    f, t = torch.cuda.mem_get_info()
    return (t - f) / 2**20


def test_calls_issued_while_the_image_is_pending(env):
    import torch
    from pollen_amd.device import DepthPlan
    n_segs = 9_000
    pools = synth.pools(61, n_segs, 12, 20_000, "pangenome")
    want = fo.seg_depth_with_uniq(pools)
    plan = DepthPlan(graph_of(pools))
    outs = [(torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0"), torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")) for _ in range(4)]
    for d, u in outs:  # (the first starts the image behind it; nothing asks for a status or a description in between)
        plan.seg_depth(d, u)
    plan.status()
    for k, (d, u) in enumerate(outs):
        assert same((d.cpu().numpy().view(np.uint32), u.cpu().numpy().view(np.uint32)), want), k
    assert IMAGE.search(plan.describe()), plan.describe()
    assert same(answers(plan, n_segs), want)
    plan.close()


def test_depth_only_and_depth_with_unique_calls_take_turns(env):
    import torch
    from pollen_amd.device import DepthPlan
    n_segs = 9_000
    pools = synth.pools(67, n_segs, 12, 20_000, "pangenome")
    want = fo.seg_depth_with_uniq(pools)
    assert (want[0] != want[1]).any() and (fo.seg_depth(pools) == want[0]).all()
    plan = DepthPlan(graph_of(pools))
    assert same(answers(plan, n_segs), want)
    assert IMAGE.search(plan.describe()), plan.describe()
    d = torch.empty(n_segs, dtype=torch.int32, device="cuda:0")
    u = torch.empty(n_segs, dtype=torch.int32, device="cuda:0")
    for k in range(6):
        d.fill_(-1)
        u.fill_(-1)
        plan.seg_depth(d, None if k % 2 == 0 else u)
        plan.status()
        assert (d.cpu().numpy().view(np.uint32) == want[0]).all(), k
        if k % 2 == 0:
            assert bool((u == -1).all()), k  # (a depth-only call leaves the unique buffer alone)
        else:
            assert (u.cpu().numpy().view(np.uint32) == want[1]).all(), k
    plan.close()


def test_plans_closed_while_their_image_is_being_made(env):
    from pollen_amd.device import DepthPlan, _lib
    n_segs = 9_000
    pools = synth.pools(71, n_segs, 12, 20_000, "pangenome")
    want = fo.seg_depth_with_uniq(pools)
    graph = graph_of(pools)
    warm = DepthPlan(graph)  # (what the library makes once and keeps is there before anything is measured)
    answers(warm, n_segs)
    warm.describe()
    warm.close()
    _lib.lib().flatgfa_dev_release_scratch()
    base = used_mb()
    for k in range(3):
        plan = DepthPlan(graph)
        assert same(answers(plan, n_segs), want), k  # (one call and its status: the image's kernels are enqueued behind it)
        plan.close()
    plan = DepthPlan(graph)
    got = [answers(plan, n_segs)]
    desc = plan.describe()
    assert IMAGE.search(desc) and PLANS_OF.search(desc).group(1) == "1", desc
    got += [answers(plan, n_segs) for _ in range(2)]
    for k, g in enumerate(got):
        assert same(g, want), k
    plan.close()
    _lib.lib().flatgfa_dev_release_scratch()
    assert abs(used_mb() - base) < 16, (base, used_mb())


def test_steps_changed_told_to_one_of_two_plans_then_the_other(env):
    import torch
    from pollen_amd.device import DepthPlan, _lib
    n_segs = 9_000
    pools = synth.pools(73, n_segs, 12, 20_000, "pangenome")
    want = fo.seg_depth_with_uniq(pools)
    graph = graph_of(pools)
    warm = DepthPlan(graph)
    answers(warm, n_segs)
    warm.describe()
    warm.close()
    _lib.lib().flatgfa_dev_release_scratch()
    base = used_mb()
    P, Q = DepthPlan(graph), DepthPlan(graph)
    for plan in (P, Q):
        assert same(answers(plan, n_segs), want)
        assert IMAGE.search(plan.describe()), plan.describe()
        assert same(answers(plan, n_segs), want)
    assert PLANS_OF.search(Q.describe()).group(1) == "2", Q.describe()
    changed = pools.steps.copy()
    changed[33_333] = (int(changed[33_333]) >> 1 ^ 4097) % n_segs << 1  # another segment, in another window
    assert int(changed[33_333]) >> 13 != int(pools.steps[33_333]) >> 13
    graph.steps[33_333] = int(changed[33_333])
    torch.cuda.synchronize()
    want = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
    P.steps_changed()
    got = [answers(P, n_segs)]
    desc = P.describe()
    assert IMAGE.search(desc) and PLANS_OF.search(desc).group(1) == "1", desc  # (a new image: Q still holds the old one)
    got += [answers(P, n_segs) for _ in range(2)]
    for k, g in enumerate(got):
        assert same(g, want), ("P", k)
    # (what Q answers between the change and being told is not specified)
    Q.steps_changed()
    got = [answers(Q, n_segs)]
    desc = Q.describe()
    assert IMAGE.search(desc) and PLANS_OF.search(desc).group(1) == "2", desc  # (... and now P's new one)
    got += [answers(Q, n_segs) for _ in range(2)] + [answers(P, n_segs)]
    for k, g in enumerate(got):
        assert same(g, want), ("Q", k)
    P.close()
    Q.close()
    _lib.lib().flatgfa_dev_release_scratch()
    assert abs(used_mb() - base) < 16, (base, used_mb())


# ---- E. refusals that guard a wrong answer ----

def test_spans_that_overlap_keep_k_scan(env):
    steps = synth.pools(79, 9_000, 1, 20_000, "pangenome").steps
    pools = make_pools(steps, [0, 6_000], [12_000, 18_000], 9_000)
    want = fo.seg_depth_with_uniq(pools)
    assert (want[0] != want[1]).any()
    desc = check(env, pools, expect_image=False, want=want)
    assert off_reason(desc) == "overlap", desc


@pytest.mark.parametrize("n_items,mean_only,verdict", [
    (100, False, "items"),      # thirteen items a workgroup, four tags
    (32, True, "image"),        # ceil(32 / 8) == 4: the rule lets it through, and FLATGFA_TAG_MEAN_ONLY lets the plan be tagged on the mean alone
    (33, True, "items"),        # ceil(33 / 8) == 5
    (32, False, "untagged"),    # what FLATGFA_TAG_LIMIT changes besides: the plan plays k_scan's deal through and wants a quarter
                                # more tags than the fullest hand (4 + 1 > 4), so without the other hook the plan is not tagged
])
def test_more_items_a_workgroup_than_it_has_private_tags(env, n_items, mean_only, verdict):
    env.setenv("FLATGFA_TAG_LIMIT", "4")
    env.setenv("FLATGFA_SCAN_WGS", "8")
    env.setenv("FLATGFA_PATH_GROUPS", "0")  # (a plan short of tags would walk the paths in groups: `ranges`)
    if mean_only:
        env.setenv("FLATGFA_TAG_MEAN_ONLY", "1")
    else:
        env.delenv("FLATGFA_TAG_MEAN_ONLY", raising=False)
    pools = synth.pools(83, 9_000, n_items, 1_000, "pangenome")
    desc = check(env, pools, expect_image=verdict == "image")
    assert " scan_workgroups=8 " in desc and " items=%d " % n_items in desc, desc
    if verdict != "image":
        assert off_reason(desc) == verdict, desc


# ---- F. the ends of the step array ----

@pytest.mark.parametrize("n_steps,tail,first_begin", [(n, t, 0) for n in (1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1) for t in (0, 5)] +
                         [(1024, 0, 1023), (2049, 0, 1023)])
def test_a_run_that_reaches_the_end_of_the_array(env, n_steps, tail, first_begin):
    # ids go up by one from step 0 to step 700, then again from a lower id to the very last step of the array (a revisit: unique
    # depth differs); the last path ends at n_steps, or five steps -- which continue its run -- before it
    ids = np.concatenate([np.arange(400, 1100), np.arange(600, 600 + n_steps - 700)]).astype(np.uint32)
    assert len(ids) == n_steps
    last = n_steps - tail
    if first_begin:
        begins, ends = ([1023], [last]) if n_steps == 1024 else ([1023, 1500], [1500, last])
    else:
        begins, ends = [0, 300], [300, last]
    pools = make_pools(ids << 1, begins, ends, 9_000)
    check(env, pools)
