"""Pass 1 from the run-length image of the steps (k_scan_runs) against the C oracle, bit for bit.

Every case makes a plan under FLATGFA_RUN_IMAGE=1 (the image whatever the graph's size and run count), FLATGFA_DEPTH_PATH=bucketed
and FLATGFA_SHORT_MAX=0 (every path an item of pass 1), makes the first call (k_scan on the steps: the image is made behind it),
asks for the description (which waits for the image and must name its size), makes two more calls (k_scan_runs on the image)
and compares all three answers with the oracle -- and with a plan of the same graph made under FLATGFA_RUN_IMAGE=0.

The graphs are small (9 000 to 300 000 segments) and shaped for what the image and the kernel can get wrong: runs that go down,
that cross window edges, that hit the 1024-step cut and the record's length limit, that end where a path ends although the ids
go on, revisits both ways, chunks of exactly 63 / 64 / 65 / 129 / 256 / 257 entries, pieces of split paths that begin and end
inside runs, more items per workgroup than the tag gate lets through at once.
"""
import dataclasses
import re

import numpy as np
import pytest

import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

HOOKS = ("FLATGFA_RUN_IMAGE", "FLATGFA_DEPTH_PATH", "FLATGFA_SHORT_MAX", "FLATGFA_PIECE_STEPS", "FLATGFA_SCAN_WGS", "FLATGFA_ACC_PARTS",
         "FLATGFA_CHECK_NO_CLAIM", "FLATGFA_RANGE_SEGS", "FLATGFA_MALL_MB", "FLATGFA_TAGGED", "FLATGFA_WB", "FLATGFA_DENSE",
         "FLATGFA_NO_CLAIM_BLOCKS_OFF", "FLATGFA_PACKED", "FLATGFA_BUCKET_CAP", "FLATGFA_TAG_LIMIT", "FLATGFA_TAG_MEAN_ONLY",
         "FLATGFA_PATH_GROUPS")
IMAGE = re.compile(r" run_image=(\d+)\b")
OFF = re.compile(r" run_image=off\((\w+)\)")


@pytest.fixture
def env(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FLATGFA_RUN_IMAGE", "1")
    monkeypatch.setenv("FLATGFA_DEPTH_PATH", "bucketed")
    monkeypatch.setenv("FLATGFA_SHORT_MAX", "0")
    # (which plans get the image is a rule; what could take it away by TIMING or by what the graph happens to earn is pinned:
    # no trial of pass 1 by partition, no per-block no-claim marks)
    monkeypatch.setenv("FLATGFA_DENSE", "0")
    monkeypatch.setenv("FLATGFA_NO_CLAIM_BLOCKS_OFF", "1")
    return monkeypatch


def make_pools(steps, begins, ends, n_segs):
    """Pools the oracle reads: `steps` (u32 handles), one path per (begin, end) span."""
    base = synth.pools(1, n_segs, 1, 1)
    paths = np.zeros(len(begins), dtype=base.paths.dtype)
    paths["steps_start"] = np.asarray(begins, dtype=np.uint64)
    paths["steps_end"] = np.asarray(ends, dtype=np.uint64)
    return dataclasses.replace(base, paths=paths, steps=np.ascontiguousarray(steps, dtype=np.uint32))


def spans_of(pools):
    return pools.paths["steps_start"].astype(np.uint32), pools.paths["steps_end"].astype(np.uint32)


def laid_out(paths, gap=0, lead=0):
    """The id lists `paths` one behind the other (`gap` unused steps between them, `lead` before the first) as forward handles."""
    steps, begins, ends = [np.zeros(lead, dtype=np.uint32)], [], []
    at = lead
    for ids in paths:
        ids = np.asarray(ids, dtype=np.uint32)
        begins.append(at)
        ends.append(at + len(ids))
        steps += [ids << 1, np.zeros(gap, dtype=np.uint32)]
        at += len(ids) + gap
    return np.concatenate(steps), begins, ends


def answers(plan, n_segs, uniq=True):
    import torch
    d = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")
    u = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0") if uniq else None
    plan.seg_depth(d, u)
    plan.status()
    return d.cpu().numpy().view(np.uint32), (u.cpu().numpy().view(np.uint32) if uniq else None)


def check(env, pools, uniq=True, expect_image=True, want=None):
    """The procedure of the module's docstring.  Returns the description of the plan with the image."""
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = len(pools.segs)
    want_d, want_u = want if want is not None else fo.seg_depth_with_uniq(pools)
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, n_segs)
    plan = DepthPlan(graph)
    got = [answers(plan, n_segs, uniq)]
    desc = plan.describe()
    if expect_image:
        assert IMAGE.search(desc), desc
    else:
        assert OFF.search(desc), desc
    got += [answers(plan, n_segs, uniq) for _ in range(2)]
    env.setenv("FLATGFA_RUN_IMAGE", "0")
    plain = DepthPlan(graph)
    env.setenv("FLATGFA_RUN_IMAGE", "1")
    got.append(answers(plain, n_segs, uniq))
    assert OFF.search(plain.describe()).group(1) == "hook", plain.describe()
    for k, (d, u) in enumerate(got):
        assert (d == want_d).all(), (k, desc, np.flatnonzero(d != want_d)[:8])
        if uniq:
            assert (u == want_u).all(), (k, desc, np.flatnonzero(u != want_u)[:8])
    plain.close()
    plan.close()
    return desc


# ---- synthetic models ----

@pytest.mark.parametrize("model,n_segs,n_paths,length", [
    ("chromosome", 20_000, 24, 30_000),   # odd paths walk the ids downwards; runs cross the edges of the 4096-segment windows
    ("pangenome", 9_000, 30, 20_000),     # revisits: unique depth differs from depth
    ("haplotype", 300_000, 12, 60_000),   # strictly monotone walks: whole-item no-claim tags
])
def test_synthetic_models(env, model, n_segs, n_paths, length):
    pools = synth.pools(7, n_segs, n_paths, length, model)
    want = fo.seg_depth_with_uniq(pools)
    if model == "pangenome":
        assert (want[0] != want[1]).any()
    desc = check(env, pools, want=want)
    if model == "haplotype":
        assert int(re.search(r"no_claim_items=(\d+)", desc).group(1)) > 0, desc


# ---- hand-made runs ----

def test_long_runs_up_and_down_meet_the_length_limit_and_the_block_cuts(env):
    # 10 000 consecutive ids up, then 10 000 down, starting off the 1024-step grid: runs of 1024 steps (a record's longest with
    # 8192-segment windows), cut at every aligned block, crossing window edges both ways
    up = np.arange(3000, 13000)
    down = np.arange(15999, 5999, -1)
    steps, b, e = laid_out([up, down], lead=5)
    check(env, make_pools(steps, b, e, 16_384))


def test_revisits_in_both_directions(env):
    ids = np.concatenate([np.arange(0, 1000), np.arange(500, 1500), np.arange(999, -1, -1)])
    steps, b, e = laid_out([ids, ids[::-1]])
    pools = make_pools(steps, b, e, 9_000)
    want = fo.seg_depth_with_uniq(pools)
    assert (want[0] != want[1]).any()
    check(env, pools, want=want)


def test_zigzags_turn_round_without_losing_or_doubling_a_step(env):
    # up-down-up every step (5 6 5 6 ...), every other step, and in blocks of three: the image's "a turn starts a run unless the
    # step before it did" rule, across a block cut as well
    a = np.tile([5, 6], 1500)
    b_ = np.tile([10, 11, 12, 11], 700)
    c = np.tile([20, 21, 22, 21, 20, 19], 500)
    steps, b, e = laid_out([a, b_, c], lead=3)
    check(env, make_pools(steps, b, e, 9_000))


# ---- path boundaries and orientation ----

def test_a_run_stops_where_its_path_ends(env):
    # every path's last id + 1 is the next path's first id, up and down, and the paths touch in the step array
    paths = [np.arange(100 * k, 100 * k + 100) for k in range(40)] + [np.arange(8999 - 50 * k, 8949 - 50 * k, -1) for k in range(40)]
    steps, b, e = laid_out(paths)
    check(env, make_pools(steps, b, e, 9_000))


def test_paths_of_no_one_and_two_steps(env):
    paths = [[], [7], [7, 8], [9, 8], [8], [], np.arange(4000, 7000), [6999], [7000, 7001]]
    steps, b, e = laid_out(paths)
    check(env, make_pools(steps, b, e, 9_000))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_step_bases_at_every_element_offset(env, offset):
    paths = [np.arange(100, 2700), np.arange(8000, 5000, -1), np.arange(2600, 4000)]
    steps, b, e = laid_out(paths, gap=1, lead=offset)
    check(env, make_pools(steps, b, e, 9_000))


def test_the_orientation_bit_is_dropped(env):
    pools = synth.pools(3, 9_000, 10, 20_000, "pangenome")
    steps = pools.steps.copy()
    steps[::3] |= 1
    steps[1::7] &= ~np.uint32(1)
    check(env, dataclasses.replace(pools, steps=steps))


# ---- chunking: a wave reads 4 x 64 entries at a time ----

@pytest.mark.parametrize("n_entries", [63, 64, 65, 129, 255, 256, 257, 1000])
def test_items_of_exact_entry_counts(env, n_entries):
    # n_entries runs of three ids with a jump between them, going up (from step 0: exactly n_entries entries while they fit the
    # first aligned block of 1024 steps, a few more where a block cut falls inside a run), and the same going down behind it
    run = np.arange(3)
    up = (np.arange(n_entries)[:, None] * 5 + run[None, :]).reshape(-1)
    down = (8990 - np.arange(n_entries)[:, None] * 5 - run[None, :]).reshape(-1)
    steps, b, e = laid_out([up, down])
    check(env, make_pools(steps, b, e, 9_000))


# ---- split paths: piece boundaries inside runs ----

@pytest.mark.parametrize("piece", [700, 1536])
def test_pieces_of_split_paths_are_clipped_to_their_steps(env, piece):
    env.setenv("FLATGFA_PIECE_STEPS", str(piece))
    env.setenv("FLATGFA_ACC_PARTS", "1")  # (split paths run tagged only where a window has one pass-2 workgroup)
    # runs of 1000 and more: whatever the piece size, boundaries fall inside runs, going up and going down
    paths = [np.arange(10, 8010), np.arange(8500, 500, -1), np.concatenate([np.arange(0, 3000), np.arange(2000, 5000)])]
    steps, b, e = laid_out(paths, lead=7)
    desc = check(env, make_pools(steps, b, e, 9_000))
    assert int(re.search(r"split_paths=(\d+)", desc).group(1)) > 0, desc


# ---- the tag gate ----

def test_more_items_per_workgroup_than_tags_in_flight(env):
    env.setenv("FLATGFA_SCAN_WGS", "96")
    pools = synth.pools(11, 300_000, 2000, 3000, "pangenome")  # 2000 items on 96 workgroups: twenty each, four tags at a time
    desc = check(env, pools)
    assert "scan_workgroups=96" in desc, desc


# ---- depth only ----

def test_depth_only_calls(env):
    pools = synth.pools(5, 20_000, 16, 30_000, "pangenome")
    want_d = fo.seg_depth(pools)
    check(env, pools, uniq=False, want=(want_d, None))


# ---- bounds ----

def test_an_id_out_of_range_is_an_error_from_the_image_too(env):
    import torch
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = 9_000
    pools = synth.pools(13, n_segs, 8, 20_000, "pangenome")
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, n_segs)
    plan = DepthPlan(graph)
    d = torch.zeros(n_segs, dtype=torch.int32, device="cuda:0")
    u = torch.zeros(n_segs, dtype=torch.int32, device="cuda:0")
    graph.steps[77_777] = (n_segs << 1) | 1  # segment id == n_segs
    torch.cuda.synchronize()
    plan.steps_changed()
    for k in range(3):  # the first from the steps, the others from the image made of the steps as they are
        plan.seg_depth(d, u)
        with pytest.raises(pa.FlatGFAError) as err:
            plan.status()
        assert err.value.code == -2, k
        if k == 0:
            assert IMAGE.search(plan.describe()), plan.describe()
    plan.close()


# ---- steps changed ----

def test_steps_changed_makes_the_image_again(env):
    import torch
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = 9_000
    pools = synth.pools(17, n_segs, 8, 20_000, "pangenome")
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, n_segs)
    plan = DepthPlan(graph)
    want = fo.seg_depth_with_uniq(pools)
    got = answers(plan, n_segs)
    assert IMAGE.search(plan.describe())
    got2 = answers(plan, n_segs)
    for d, u in (got, got2):
        assert (d == want[0]).all() and (u == want[1]).all()
    changed = pools.steps.copy()
    changed[33_333] = (int(changed[33_333]) >> 1 ^ 4097) % n_segs << 1  # another segment, in another window
    graph.steps[33_333] = int(changed[33_333])
    torch.cuda.synchronize()
    plan.steps_changed()
    want = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
    got = answers(plan, n_segs)
    assert IMAGE.search(plan.describe()), plan.describe()
    for d, u in (got, answers(plan, n_segs), answers(plan, n_segs)):
        assert (d == want[0]).all() and (u == want[1]).all()
    plan.close()


def test_no_image_while_the_plan_checks_its_facts(env):
    env.setenv("FLATGFA_CHECK_NO_CLAIM", "1")
    pools = synth.pools(19, 9_000, 8, 20_000, "haplotype")
    from pollen_amd.device import DepthPlan, DeviceGraph
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, 9_000)
    plan = DepthPlan(graph)
    want = fo.seg_depth_with_uniq(pools)
    got = [answers(plan, 9_000)]
    assert OFF.search(plan.describe()).group(1) == "check_no_claim", plan.describe()
    got.append(answers(plan, 9_000))
    for d, u in got:
        assert (d == want[0]).all() and (u == want[1]).all()
    plan.close()


# ---- plans that are not given one ----

@pytest.mark.parametrize("how,reason", [("short", "short_paths"), ("ranges", "ranges")])
def test_ineligible_plans_say_why_and_count_right(env, how, reason):
    if how == "short":
        env.delenv("FLATGFA_SHORT_MAX")  # paths of 300 steps beside the long ones: a wave-per-path list
        long_ = synth.pools(23, 9_000, 6, 20_000, "pangenome")
        short = synth.pools(29, 9_000, 200, 300, "pangenome")
        steps = np.concatenate([long_.steps, short.steps])
        begins = list(range(0, 120_000, 20_000)) + list(range(120_000, 180_000, 300))
        ends = [b + 20_000 for b in begins[:6]] + [b + 300 for b in begins[6:]]
        pools = make_pools(steps, begins, ends, 9_000)
    else:
        env.setenv("FLATGFA_RANGE_SEGS", "40960")
        pools = synth.pools(31, 100_000, 8, 30_000, "pangenome")
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    plan = DepthPlan(DeviceGraph(pools.steps, begins, ends, n_segs))
    want = fo.seg_depth_with_uniq(pools)
    got = [answers(plan, n_segs)]
    desc = plan.describe()
    assert OFF.search(desc) and OFF.search(desc).group(1) == reason, desc
    got.append(answers(plan, n_segs))
    for d, u in got:
        assert (d == want[0]).all() and (u == want[1]).all()
    plan.close()


# ---- one image for all the plans of a step array ----

def test_a_pipeline_and_a_plan_share_one_image(env):
    """Three lanes and a stand-alone plan on one graph: device memory grows by ONE image over the same four plans without
    (16 MB tolerance, as the scratch test's; the image is 10 MB here, so four would show), every lane's answers are exact, and the
    memory is back once the plans are closed."""
    import torch
    from pollen_amd.device import DepthPipeline, DepthPlan, DeviceGraph, _lib
    n_segs, n_paths, length = 300_000, 40, 128_000
    env.setenv("FLATGFA_ACC_PARTS", "1")  # (paths this long are cut into pieces, which run tagged only where a window has one pass-2 workgroup)
    # runs of four ids: 1.28 M entries of 8 bytes in 5.12 M steps
    starts = (synth.mix64(np.arange(n_paths * length // 4, dtype=np.uint64) * synth.GOLDEN) % np.uint64(n_segs - 4)).astype(np.uint32)
    ids = (starts[:, None] + np.arange(4, dtype=np.uint32)[None, :]).reshape(-1)
    begins = np.arange(n_paths, dtype=np.uint32) * length
    pools = make_pools(ids << 1, begins, begins + length, n_segs)
    want = fo.seg_depth_with_uniq(pools)
    graph = DeviceGraph(pools.steps, begins, begins + length, n_segs)
    bufs = [torch.zeros(2 * n_segs, dtype=torch.int32, device="cuda:0") for _ in range(4)]

    def used():
        torch.cuda.synchronize()
        f, t = torch.cuda.mem_get_info()
        return (t - f) / 2**20

    def run(image):
        env.setenv("FLATGFA_RUN_IMAGE", "1" if image else "0")
        pipe, plan = DepthPipeline(graph, 3), DepthPlan(graph)
        mb = None
        for rnd in range(3):
            for k in range(3):
                pipe.seg_depth(bufs[k][:n_segs], bufs[k][n_segs:])
            pipe.status()
            plan.seg_depth(bufs[3][:n_segs], bufs[3][n_segs:])
            plan.status()
            for b in bufs:
                got = b.cpu().numpy().view(np.uint32)
                assert (got[:n_segs] == want[0]).all() and (got[n_segs:] == want[1]).all(), (image, rnd)
            desc, pdesc = plan.describe(), pipe.describe()
            if image:
                assert IMAGE.search(desc) and IMAGE.search(pdesc), (desc, pdesc)
                mb = int(IMAGE.search(desc).group(1))
            else:
                assert OFF.search(desc).group(1) == "hook" and OFF.search(pdesc).group(1) == "hook"
        there = used()
        pipe.close()
        plan.close()
        _lib.lib().flatgfa_dev_release_scratch()
        return there, mb

    run(False)  # (what the library makes once and keeps -- its streams, its staging memory -- is there before anything is measured)
    _lib.lib().flatgfa_dev_release_scratch()
    base = used()
    without, _ = run(False)
    assert abs(used() - base) < 16, (base, used())
    with_image, mb = run(True)
    assert 9 <= mb <= 12, mb
    assert abs((with_image - without) - mb) < 16, (base, without, with_image, mb)
    assert abs(used() - base) < 16, (base, used())   # (the last plan to go freed it)
