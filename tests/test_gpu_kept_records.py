"""Pass 1's records kept across calls: an image call behind another image call of the same plan runs
pass 2 alone, on the records k_scan_runs left in the plan's scratch -- against the C oracle, bit for bit, in buffers pre-filled
with -1, and with the kernels each call launched taken from the library's own profile (device.profile_enable / profile_read).

The environment is test_gpu_run_image.py's: FLATGFA_RUN_IMAGE=1 (the image whatever the graph's size), the bucketed path, every
path an item of pass 1, no pass 1 by partition, no per-block marks.  Every case makes a plan, makes the first call (k_scan on
the steps: the image is made behind it) and asks for the description, which waits for the image and says ` records=kept`; what
follows is the case's own.  What the cases are after: the state is kept where it may be (calls with no status between them,
calls of either mode, two plans on one step array, lanes of a pipeline) and dropped where it must be (a call in another mode, a
status that reads an error or a sub-bucket more than half full, changed steps), and a kept call zeroes what pass 1 would have
zeroed (two pass-2 workgroups per window).
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
         "FLATGFA_PATH_GROUPS", "FLATGFA_KEEP_RECORDS")
IMAGE = re.compile(r" run_image=(\d+)\b")
RECORDS = re.compile(r" records=(kept|rewritten)$")


@pytest.fixture
def env(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FLATGFA_RUN_IMAGE", "1")
    monkeypatch.setenv("FLATGFA_DEPTH_PATH", "bucketed")
    monkeypatch.setenv("FLATGFA_SHORT_MAX", "0")
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


def laid_out(paths, lead=0):
    """The id lists `paths` one behind the other (`lead` unused steps before the first) as forward handles."""
    steps, begins, ends = [np.zeros(lead, dtype=np.uint32)], [], []
    at = lead
    for ids in paths:
        ids = np.asarray(ids, dtype=np.uint32)
        begins.append(at)
        ends.append(at + len(ids))
        steps.append(ids << 1)
        at += len(ids)
    return np.concatenate(steps), begins, ends


_WANT = {}


def synth_case(seed, n_segs, n_paths, length, model):
    """A synthetic graph and the oracle's answer for it, computed once and shared (nobody writes to either)."""
    key = (seed, n_segs, n_paths, length, model)
    if key not in _WANT:
        pools = synth.pools(seed, n_segs, n_paths, length, model)
        _WANT[key] = (pools, fo.seg_depth_with_uniq(pools))
    return _WANT[key]


def buffers(n_segs, uniq=True):
    import torch
    d = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")
    return d, (torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0") if uniq else None)


def assert_right(bufs, want, what):
    d, u = bufs
    got = d.cpu().numpy().view(np.uint32)
    assert (got == want[0]).all(), (what, "depth", np.flatnonzero(got != want[0])[:8])
    if u is not None:
        got = u.cpu().numpy().view(np.uint32)
        assert (got == want[1]).all(), (what, "uniq", np.flatnonzero(got != want[1])[:8])


def first_call(plan, n_segs, want, expect="kept"):
    """The plan's first call (k_scan on the steps), checked, and its description once the image is there."""
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call")
    desc = plan.describe()
    assert IMAGE.search(desc), desc
    assert RECORDS.search(desc) and RECORDS.search(desc).group(1) == expect, desc
    return desc


class Profile:
    """The kernels the library launched inside the `with` block, by name."""

    def __enter__(self):
        from pollen_amd import device as dev
        dev.profile_enable(True)
        dev.profile_read()
        self.names = []
        return self

    def __exit__(self, *exc):
        import torch
        from pollen_amd import device as dev
        torch.cuda.synchronize()
        self.names = [n for n, _ in dev.profile_read()]
        dev.profile_enable(False)
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)

    def pass1(self):
        return sum(1 for n in self.names if n.startswith("k_scan"))

    def pass2(self):
        return sum(1 for n in self.names if n.startswith("k_accum"))


def five_calls(plan, n_segs, want, runs=1, uniq=True):
    """Five calls with no status between them, into five pairs of buffers; then the status.  One k_scan_runs (none: runs=0), five k_accum."""
    bufs = [buffers(n_segs, uniq) for _ in range(5)]
    with Profile() as prof:
        for b in bufs:
            plan.seg_depth(*b)
        plan.status()
    for k, b in enumerate(bufs):
        assert_right(b, want, f"call {k} of five")
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (runs, runs, 5), prof.names
    return prof


def plan_of(pools, seg_len=False):
    """The graph on the device (with the segments' lengths: `seg_len`), a plan for it, the number of segments."""
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    lens = np.ascontiguousarray(pools.seg_lens(), dtype=np.uint32) if seg_len else None
    graph = DeviceGraph(pools.steps, begins, ends, n_segs, lens)
    return graph, DepthPlan(graph), n_segs


# ---- five calls with no status between them ----

@pytest.mark.parametrize("model,n_segs,n_paths,length", [
    ("pangenome", 9_000, 30, 20_000),     # revisits: unique depth differs from depth
    ("chromosome", 20_000, 24, 30_000),   # runs cross the edges of the windows, odd paths walk downwards
    ("haplotype", 300_000, 12, 60_000),   # strictly monotone walks: no-claim tags
])
def test_five_calls_run_pass_1_once(env, model, n_segs, n_paths, length):
    pools, want = synth_case(7, n_segs, n_paths, length, model)
    if model == "pangenome":
        assert (want[0] != want[1]).any()
    _, plan, _ = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    if model == "haplotype":
        assert int(re.search(r"no_claim_items=(\d+)", desc).group(1)) > 0, desc
    five_calls(plan, n_segs, want)
    # a clean status drops nothing; one that found a sub-bucket more than half full gave the plan larger buckets, which shows
    cap = lambda text: int(re.search(r"bucket_cap=(\d+)", text).group(1))
    five_calls(plan, n_segs, want, runs=0 if cap(plan.describe()) == cap(desc) else 1)
    five_calls(plan, n_segs, want, runs=0)  # (... once: what was more than half full is at most half full then)
    plan.close()


def test_five_calls_on_a_split_path(env):
    env.setenv("FLATGFA_PIECE_STEPS", "700")
    env.setenv("FLATGFA_ACC_PARTS", "1")  # (split paths run tagged only where a window has one pass-2 workgroup)
    paths = [np.arange(10, 8010), np.arange(8500, 500, -1), np.concatenate([np.arange(0, 3000), np.arange(2000, 5000)])]
    steps, b, e = laid_out(paths, lead=7)
    pools = make_pools(steps, b, e, 9_000)
    want = fo.seg_depth_with_uniq(pools)
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert int(re.search(r"split_paths=(\d+)", desc).group(1)) > 0, desc  # (shared tags: bitsets all waves of a window's workgroup use)
    five_calls(plan, n_segs, want)
    plan.close()


def test_five_calls_with_fewer_items_than_sub_buckets(env):
    """Two paths: pass 1 runs two workgroups and writes two cursors per window; pass 2 reads a cursor for every sub-bucket of
    the window, and those of the others must read zero in the kept copy as well (runs of 1024 steps up and down, which cross
    the windows' edges: a record at a window's first segment is what a stray cursor would count)."""
    # (a plan of as many windows and thirty items goes first: the block its kept cursors lay in is free, and full of them, when
    # the plan under test asks for one of the same size)
    other, other_want = synth_case(7, 16_384, 30, 20_000, "pangenome")
    _, plan, n_segs = plan_of(other)
    first_call(plan, n_segs, other_want)
    five_calls(plan, n_segs, other_want)
    plan.close()
    up = np.arange(3000, 13000)
    down = np.arange(15999, 5999, -1)
    steps, b, e = laid_out([up, down], lead=5)
    pools = make_pools(steps, b, e, 16_384)
    want = fo.seg_depth_with_uniq(pools)
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert "items=2 " in desc and "scan_workgroups=2 " not in desc, desc
    five_calls(plan, n_segs, want)
    plan.close()


def test_five_calls_with_few_pass_1_workgroups(env):
    env.setenv("FLATGFA_SCAN_WGS", "96")
    pools, want = synth_case(11, 300_000, 2000, 3000, "pangenome")  # 2000 items on 96 workgroups: twenty each, so bitsets change hands
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert "scan_workgroups=96" in desc, desc
    five_calls(plan, n_segs, want)
    plan.close()


@pytest.mark.parametrize("wb", [11, 12, 13])
def test_five_calls_at_every_window_width(env, wb):
    env.setenv("FLATGFA_WB", str(wb))
    pools, want = synth_case(7, 20_000, 24, 30_000, "chromosome")
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert f"x{1 << wb} " in desc, desc
    five_calls(plan, n_segs, want)
    plan.close()


def test_a_kept_call_zeroes_the_outputs_two_workgroups_add_to(env):
    """Two pass-2 workgroups per window ADD to the outputs, which pass 1 zeroes on its way: a call without pass 1 has to do that
    itself, or the -1 the buffers are filled with (and, on a second use, the answer before) stays in the sum."""
    env.setenv("FLATGFA_ACC_PARTS", "2")
    pools, want = synth_case(7, 9_000, 30, 20_000, "pangenome")
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert "workgroups_per_window=2" in desc, desc
    five_calls(plan, n_segs, want)
    b = buffers(n_segs)
    for k in range(3):  # ... and into buffers that hold an answer already
        plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "the same buffers three times")
    plan.close()


# ---- either mode reads the same records ----

def test_calls_of_both_modes_share_the_records(env):
    pools, want = synth_case(7, 9_000, 30, 20_000, "pangenome")
    _, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    a, b, c = buffers(n_segs), buffers(n_segs, uniq=False), buffers(n_segs)
    with Profile() as prof:
        plan.seg_depth(*a)
        plan.seg_depth(*b)
        plan.seg_depth(*c)
        plan.status()
    for k, x in enumerate((a, b, c)):
        assert_right(x, want, k)
    assert (prof.count("k_scan_runs"), prof.pass1()) == (1, 1), prof.names
    assert (prof.count("k_accum<uniq>"), prof.count("k_accum<depth>")) == (2, 1), prof.names
    plan.close()


# ---- what drops the state ----

def test_a_call_in_another_mode_overwrites_the_records(env):
    """path_depth_all runs k_scan (its records carry no tags) into the same buckets: the image call behind it runs pass 1 again,
    the one after that does not.  (One pass-2 workgroup per window: with more, path_depth_all is a depth call and a gather, and
    its depth call may use the records like any other.)"""
    import torch
    from pollen_amd.device import DepthPlan, DeviceGraph
    env.setenv("FLATGFA_ACC_PARTS", "1")
    pools, want = synth_case(7, 9_000, 30, 20_000, "pangenome")
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    seg_len = np.ascontiguousarray(pools.seg_lens(), dtype=np.uint32)
    plan = DepthPlan(DeviceGraph(pools.steps, begins, ends, n_segs, seg_len))
    first_call(plan, n_segs, want)
    a, c, e = buffers(n_segs), buffers(n_segs), buffers(n_segs)
    d = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")
    ln = torch.full((len(begins),), -1, dtype=torch.int64, device="cuda:0")
    ws = torch.full((len(begins),), -1, dtype=torch.int64, device="cuda:0")
    with Profile() as prof:
        plan.seg_depth(*a)
        plan.path_depth_all(d, ln, ws)
        plan.seg_depth(*c)
        plan.seg_depth(*e)
        plan.status()
    for k, x in enumerate((a, c, e)):
        assert_right(x, want, k)
    assert_right((d, None), want, "path_depth_all's depth")
    ids = pools.steps >> 1
    lens = seg_len.astype(np.uint64)
    want_ln = np.array([lens[ids[b:e_]].sum() for b, e_ in zip(begins, ends)], dtype=np.uint64)
    want_ws = np.array([(want[0][ids[b:e_]].astype(np.uint64) * lens[ids[b:e_]]).sum() for b, e_ in zip(begins, ends)], dtype=np.uint64)
    assert (ln.cpu().numpy().view(np.uint64) == want_ln).all() and (ws.cpu().numpy().view(np.uint64) == want_ws).all()
    assert (prof.count("k_scan_runs"), prof.count("k_scan")) == (2, 1), prof.names
    plan.close()


def test_steps_changed_drops_the_records(env):
    import torch
    pools, want = synth_case(17, 9_000, 8, 20_000, "pangenome")
    graph, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    five_calls(plan, n_segs, want)
    changed = pools.steps.copy()
    at = np.arange(1000, 150_000, 997)
    changed[at] = ((changed[at] >> 1 ^ 4097) % n_segs << 1).astype(np.uint32)  # other segments, in other windows
    graph.steps[torch.from_numpy(at).to("cuda:0")] = torch.from_numpy(changed[at].view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    plan.steps_changed()
    want2 = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
    assert (want2[0] != want[0]).any()
    first_call(plan, n_segs, want2)
    five_calls(plan, n_segs, want2)
    plan.close()


def test_an_id_out_of_range_is_an_error_in_every_round(env):
    """Only pass 1 sees the steps: a status that reads the error drops the records, so the next call raises it again."""
    import torch
    pools, _ = synth_case(13, 9_000, 8, 20_000, "pangenome")
    graph, plan, n_segs = plan_of(pools)
    d, u = buffers(n_segs)
    graph.steps[77_777] = (n_segs << 1) | 1  # segment id == n_segs
    torch.cuda.synchronize()
    plan.steps_changed()
    for k in range(4):  # the first from the steps, the others from the image
        with Profile() as prof:
            plan.seg_depth(d, u)
            with pytest.raises(pa.FlatGFAError) as err:
                plan.status()
        assert err.value.code == -2, k
        if k == 0:
            desc = plan.describe()
            assert IMAGE.search(desc) and RECORDS.search(desc).group(1) == "kept", desc
        else:
            assert prof.count("k_scan_runs") == 1, (k, prof.names)
    graph.steps[77_777] = int(pools.steps[77_777])  # (the graph's tensor is the test's own; put back for tidiness)
    plan.close()


def test_a_sub_bucket_more_than_half_full_drops_the_records(env):
    """One path of 640 runs and seven of 40, all in the first window, in sub-buckets of 1024 records (FLATGFA_BUCKET_CAP, which
    also pins the capacity: the status cannot grow the plan here, but it reads the fullest word and must take the buckets for
    changed).  Whatever the deal, a sub-bucket holds between 640 and 920 records: more than half, never too many."""
    env.setenv("FLATGFA_BUCKET_CAP", "1024")
    run = np.arange(4)
    paths = [(np.arange(640)[:, None] * 5 + run[None, :]).reshape(-1)] + [(np.arange(40)[:, None] * 7 + 11 * k + run[None, :]).reshape(-1) for k in range(7)]
    steps, b, e = laid_out(paths)
    pools = make_pools(steps, b, e, 9_000)
    want = fo.seg_depth_with_uniq(pools)
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert "bucket_cap=1024" in desc, desc
    bufs = [buffers(n_segs) for _ in range(4)]
    with Profile() as prof:
        plan.seg_depth(*bufs[0])
        plan.seg_depth(*bufs[1])
        plan.status()  # (reads a fullest sub-bucket beyond half the capacity)
        plan.seg_depth(*bufs[2])
        plan.seg_depth(*bufs[3])
        plan.status()
    for k, x in enumerate(bufs):
        assert_right(x, want, k)
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (2, 2, 4), prof.names
    plan.close()


# ---- every plan its own records ----

def test_two_plans_on_one_step_array_keep_their_own_records(env):
    from pollen_amd.device import DepthPlan, DeviceGraph
    pools, want = synth_case(7, 9_000, 30, 20_000, "pangenome")
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, n_segs)
    some = np.arange(0, len(begins), 3)
    sub = DeviceGraph.from_tensors(graph.steps, graph.path_begin[::3].contiguous(), graph.path_end[::3].contiguous(), n_segs)
    want_sub = fo.seg_depth_with_uniq(make_pools(pools.steps, begins[some], ends[some], n_segs))
    assert (want_sub[0] != want[0]).any()
    plan, plan_sub = DepthPlan(graph), DepthPlan(sub)
    first_call(plan, n_segs, want)
    desc = first_call(plan_sub, n_segs, want_sub)
    assert "run_image_plans=2" in desc, desc
    bufs = [buffers(n_segs) for _ in range(6)]
    with Profile() as prof:
        for k, b in enumerate(bufs):
            (plan_sub if k % 2 else plan).seg_depth(*b)
        plan.status()
        plan_sub.status()
    for k, b in enumerate(bufs):
        assert_right(b, want_sub if k % 2 else want, k)
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (2, 2, 6), prof.names
    plan_sub.close()
    plan.close()


def test_every_lane_of_a_pipeline_keeps_its_own_records(env):
    from pollen_amd.device import DepthPipeline, DeviceGraph
    pools, want = synth_case(7, 20_000, 24, 30_000, "chromosome")
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    pipe = DepthPipeline(DeviceGraph(pools.steps, begins, ends, n_segs), 3)
    warm = [buffers(n_segs) for _ in range(3)]
    for b in warm:
        pipe.seg_depth(*b)
    pipe.status()
    for b in warm:
        assert_right(b, want, "first round")
    desc = pipe.describe()
    assert IMAGE.search(desc) and RECORDS.search(desc).group(1) == "kept", desc
    bufs = [buffers(n_segs) for _ in range(9)]
    with Profile() as prof:
        for b in bufs:
            pipe.seg_depth(*b)
        pipe.status()
    for k, b in enumerate(bufs):
        assert_right(b, want, k)
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (3, 3, 9), prof.names
    pipe.close()


# ---- the hook ----

def test_with_the_hook_off_every_call_runs_pass_1(env):
    env.setenv("FLATGFA_KEEP_RECORDS", "0")
    pools, want = synth_case(7, 9_000, 30, 20_000, "pangenome")
    _, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want, expect="rewritten")
    five_calls(plan, n_segs, want, runs=5)
    plan.close()
