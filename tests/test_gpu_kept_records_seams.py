"""Pass 1's kept records at the seams test_gpu_kept_records.py leaves out: the plan's other calls between
kept calls (path_depth_all as a kept call itself; path_sums and path_overlaps, which use the plan and its status word but not
its buckets; a bad query id, which is a status like any other), a plan handed from stream to stream, pipelines whose lanes
take calls of every kind, get their steps changed or read an error, the host handles that call into buffers of their own
again and again (a resident FlatGFA with its subset plan, the shards of a ShardedFlatGFA), and the plan nobody forced: no
hooks, the image by the graph's size.

As there: depth and unique depth against the C oracle, bit for bit, in buffers pre-filled with -1 where the test owns them;
path lengths and weighted sums against uint64 sums in numpy, overlaps against set intersections in numpy; the kernels a
block launched from the library's own profile.  A call of a plan through the bucketed kernels launches one k_accum and at
most one k_scan*: a block with fewer k_scan* than k_accum has run on kept records.
"""
import dataclasses
import re

import numpy as np
import pytest

import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from test_gpu_kept_records import (HOOKS, IMAGE, RECORDS, Profile, assert_right, buffers, env, first_call, five_calls, laid_out,  # noqa: F401
                                   make_pools, plan_of, spans_of, synth_case)

pytestmark = pytest.mark.gpu

PANGENOME = (7, 9_000, 30, 20_000, "pangenome")
CHROMOSOME = (7, 20_000, 24, 30_000, "chromosome")


def sums_of(pools, depth, ids=None):
    """measure_path's two integer sums of the paths `ids` (all of them: None) against `depth`, in uint64."""
    begins, ends = spans_of(pools)
    seg = pools.steps >> 1
    lens = pools.seg_lens().astype(np.uint64)
    ids = range(len(begins)) if ids is None else ids
    ln = np.array([lens[seg[begins[p]:ends[p]]].sum() for p in ids], dtype=np.uint64)
    ws = np.array([(depth[seg[begins[p]:ends[p]]].astype(np.uint64) * lens[seg[begins[p]:ends[p]]]).sum() for p in ids], dtype=np.uint64)
    return ln, ws


def touches_of(pools, queries):
    """touch[k, j]: path j has a handle in common with path queries[k], and is another path."""
    begins, ends = spans_of(pools)
    sets = [np.unique(pools.steps[b:e]) for b, e in zip(begins, ends)]
    out = np.zeros((len(queries), len(sets)), dtype=np.uint8)
    for k, q in enumerate(queries):
        for j, s in enumerate(sets):
            out[k, j] = j != q and len(np.intersect1d(sets[q], s, assume_unique=True)) > 0
    return out


def sum_buffers(n_paths):
    import torch
    return (torch.full((n_paths,), -1, dtype=torch.int64, device="cuda:0"), torch.full((n_paths,), -1, dtype=torch.int64, device="cuda:0"))


def assert_sums(got, want, what):
    for name, g, w in zip(("lengths", "weighted sums"), got, want):
        g = g.cpu().numpy().view(np.uint64)
        assert (g == w).all(), (what, name, np.flatnonzero(g != w)[:8])


# ---- A. the plan's other calls between kept calls ----

@pytest.mark.parametrize("parts,wb,case", [(2, 12, PANGENOME), (1, 11, CHROMOSOME), (1, 13, CHROMOSOME)], ids=["parts2-wb12", "parts1-wb11", "parts1-wb13"])
def test_path_depth_all_runs_on_kept_records(env, parts, wb, case):
    """Two pass-2 workgroups per window, or windows of another width than 4096: pass 2 does not add the paths up
    (fast_plan_want_path_sums), path_depth_all is a tagged depth call and a gather -- an image call like any other, which reads
    the records and leaves them.  Its second call writes where its first one wrote: with two workgroups per window, sums."""
    env.setenv("FLATGFA_ACC_PARTS", str(parts))
    env.setenv("FLATGFA_WB", str(wb))
    pools, want = synth_case(*case)
    assert (want[0] != want[1]).any()
    _, plan, n_segs = plan_of(pools, seg_len=True)
    desc = first_call(plan, n_segs, want)
    assert f"workgroups_per_window={parts} " in desc and f"x{1 << wb} " in desc, desc
    want_sums = sums_of(pools, want[0])
    a, c, e = buffers(n_segs), buffers(n_segs), buffers(n_segs, uniq=False)
    d, _ = buffers(n_segs, uniq=False)
    sums = sum_buffers(len(pools.paths))
    with Profile() as prof:
        plan.seg_depth(*a)
        plan.path_depth_all(d, *sums)
        first = (d.clone(), sums[0].clone(), sums[1].clone())  # (on the calls' stream, between them)
        plan.seg_depth(*c)
        plan.path_depth_all(d, *sums)
        plan.seg_depth(*e)
        plan.status()
    for k, x in enumerate((a, c, e)):
        assert_right(x, want, ("seg_depth", k))
    assert_right((first[0], None), want, "the first path_depth_all's depth")
    assert_sums(first[1:], want_sums, "the first path_depth_all")
    assert_right((d, None), want, "the second path_depth_all's depth")
    assert_sums(sums, want_sums, "the second path_depth_all")
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (1, 1, 5), prof.names
    assert (prof.count("k_accum<uniq>"), prof.count("k_accum<depth>"), prof.count("k_path_sums")) == (2, 3, 2), prof.names
    # (what a kept call's workgroups add to is zeroed by the call: four kept calls; one workgroup per window stores)
    assert prof.count("memset_outputs") == (4 if parts > 1 else 0), prof.names
    plan.close()


@pytest.mark.parametrize("parts", [None, "2"])
def test_path_sums_and_path_overlaps_leave_the_records_alone(env, parts):
    import torch
    if parts:
        env.setenv("FLATGFA_ACC_PARTS", parts)
    pools, want = synth_case(*PANGENOME)
    n_paths = len(pools.paths)
    _, plan, n_segs = plan_of(pools, seg_len=True)
    first_call(plan, n_segs, want)
    ids = np.arange(1, n_paths, 4)
    queries = [0, 7, n_paths - 1]
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda:0")
    d_q = torch.tensor(queries, dtype=torch.int32, device="cuda:0")
    sums = sum_buffers(len(ids))
    touch = torch.full((len(queries) * n_paths,), 255, dtype=torch.uint8, device="cuda:0")
    a, b, c = buffers(n_segs), buffers(n_segs), buffers(n_segs)
    with Profile() as prof:
        plan.seg_depth(*a)
        plan.path_sums(d_ids, a[0], *sums)
        plan.seg_depth(*b)
        plan.path_overlaps(d_q, touch)
        plan.seg_depth(*c)
        plan.status()
    for k, x in enumerate((a, b, c)):
        assert_right(x, want, k)
    assert_sums(sums, sums_of(pools, want[0], ids), "path_sums")
    got = touch.cpu().numpy().reshape(len(queries), n_paths)
    want_touch = touches_of(pools, queries)
    assert want_touch.any() and not want_touch.all()
    assert (got == want_touch).all(), np.argwhere(got != want_touch)[:8]
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (1, 1, 3), prof.names
    assert prof.count("k_path_sums") == 1 and prof.count("k_pair_touch") == 1, prof.names
    plan.close()


def test_a_bad_query_id_drops_the_records(env):
    """path_overlaps reports a query id out of range through the plan's status word: the status that reads it drops the records,
    as it does for any word but zero."""
    import torch
    pools, want = synth_case(*PANGENOME)
    n_paths = len(pools.paths)
    _, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    a, b, c, d = (buffers(n_segs) for _ in range(4))
    d_q = torch.tensor([3, n_paths, 5], dtype=torch.int32, device="cuda:0")
    touch = torch.full((3 * n_paths,), 255, dtype=torch.uint8, device="cuda:0")
    with Profile() as prof:
        plan.seg_depth(*a)
        plan.seg_depth(*b)
        plan.path_overlaps(d_q, touch)
        with pytest.raises(pa.FlatGFAError) as err:
            plan.status()
    assert err.value.code == -2
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (1, 1, 2), prof.names
    assert_right(a, want, "before the bad query, 0")
    assert_right(b, want, "before the bad query, 1")
    with Profile() as prof:
        plan.seg_depth(*c)
        plan.seg_depth(*d)
        plan.status()
    assert_right(c, want, "behind the error, 0")
    assert_right(d, want, "behind the error, 1")
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (1, 1, 2), prof.names
    plan.close()


# ---- B. streams ----

def test_a_plan_moved_between_streams_keeps_its_records(env):
    """Calls of one plan must not overlap in time; they need not share a stream.  With an event between them, a kept call on
    another stream than pass 1's reads complete records."""
    import torch
    pools, want = synth_case(*PANGENOME)
    _, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = [buffers(n_segs) for _ in range(3)]  # (alive to the end: torch's allocator hands nothing of them on)
    calls = [plan.seg_depth_call(*bufs[0], stream=s1), plan.seg_depth_call(*bufs[1], stream=s2), plan.seg_depth_call(*bufs[2], stream=s1)]
    torch.cuda.synchronize()  # (the fills ran on the current stream)
    with Profile() as prof:
        calls[0]()
        s2.wait_stream(s1)
        calls[1]()
        s1.wait_stream(s2)
        calls[2]()
        torch.cuda.synchronize()
        plan.status()
    for k, b in enumerate(bufs):
        assert_right(b, want, ("stream", k))
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (1, 1, 3), prof.names
    plan.close()


# ---- C. pipelines ----

KINDS = ("seg_depth(d,u)", "seg_depth(d)", "path_depth_all")


def pipeline_of(env, pools):
    from pollen_amd.device import DepthPipeline, DeviceGraph
    env.setenv("FLATGFA_ACC_PARTS", "2")  # (path_depth_all is a depth call and a gather: it may keep)
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, len(pools.segs), np.ascontiguousarray(pools.seg_lens(), dtype=np.uint32))
    return graph, DepthPipeline(graph, 3)


def warm_round(pipe, n_segs, want):
    """Every lane's first call (k_scan on the steps), and the description once every lane has the image."""
    warm = [buffers(n_segs) for _ in range(3)]
    for b in warm:
        pipe.seg_depth(*b)
    pipe.status()
    for b in warm:
        assert_right(b, want, "warm round")
    desc = pipe.describe()
    assert IMAGE.search(desc) and RECORDS.search(desc).group(1) == "kept", desc
    assert "workgroups_per_window=2 " in desc, desc
    return desc


def mixed_calls(pipe, pools, want, n, shift=0):
    """`n` calls that cycle through the three kinds (from kind `shift` on), every second one without waiting for the current
    stream; join, the answers read on the current stream, then the status.  All answers checked; returns the profile."""
    import torch
    n_segs, n_paths = len(pools.segs), len(pools.paths)
    want_sums = sums_of(pools, want[0])
    kinds = [(k + shift) % 3 for k in range(n)]
    bufs = [buffers(n_segs, uniq=kind == 0) + (sum_buffers(n_paths) if kind == 2 else ()) for kind in kinds]
    torch.cuda.synchronize()  # (a call that does not wait for the current stream must not overtake the fills)
    with Profile() as prof:
        for k, (kind, b) in enumerate(zip(kinds, bufs)):
            if kind == 2:
                pipe.path_depth_all(b[0], b[2], b[3], after_current_stream=k % 2 == 0)
            else:
                pipe.seg_depth(b[0], b[1], after_current_stream=k % 2 == 0)
        pipe.join()
        got = [tuple(None if t is None else t.cpu() for t in b) for b in bufs]  # (the current stream waits for every lane)
        pipe.status()
    for k, (kind, g) in enumerate(zip(kinds, got)):
        assert_right(g[:2], want, (k, KINDS[kind]))
        if kind == 2:
            assert_sums(g[2:], want_sums, (k, KINDS[kind]))
    return prof


def test_ten_mixed_calls_on_a_pipeline_run_pass_1_once_a_lane(env):
    pools, want = synth_case(*CHROMOSOME)
    _, pipe = pipeline_of(env, pools)
    warm_round(pipe, len(pools.segs), want)
    prof = mixed_calls(pipe, pools, want, 10)  # (ten is no multiple of three: lane 0 takes four)
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (3, 3, 10), prof.names
    assert prof.count("k_path_sums") == 3, prof.names
    pipe.close()


def changed_steps(pools, graph):
    """Other step values on the device (as test_steps_changed_drops_the_records) and the pools that have them."""
    import torch
    n_segs = len(pools.segs)
    changed = pools.steps.copy()
    at = np.arange(1000, 150_000, 997)
    changed[at] = ((changed[at] >> 1 ^ 4097) % n_segs << 1).astype(np.uint32)  # other segments, in other windows
    graph.steps[torch.from_numpy(at).to("cuda:0")] = torch.from_numpy(changed[at].view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return dataclasses.replace(pools, steps=changed)


def test_steps_changed_on_a_pipeline_drops_every_lanes_records(env):
    pools, want = synth_case(*CHROMOSOME)
    n_segs = len(pools.segs)
    graph, pipe = pipeline_of(env, pools)
    warm_round(pipe, n_segs, want)
    mixed_calls(pipe, pools, want, 10)  # (every lane holds records of the old steps, and the next call is lane 1's)
    pools2 = changed_steps(pools, graph)
    pipe.steps_changed()
    want2 = fo.seg_depth_with_uniq(pools2)
    assert (want2[0] != want[0]).any()
    warm_round(pipe, n_segs, want2)
    prof = mixed_calls(pipe, pools2, want2, 6, shift=1)  # (each lane another kind than before)
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (3, 3, 6), prof.names
    pipe.close()


def test_an_id_out_of_range_is_an_error_in_every_round_of_a_pipeline(env):
    """Only pass 1 sees the steps, and every lane's status reads the error: no lane keeps records behind it."""
    import torch
    pools, want = synth_case(*CHROMOSOME)
    n_segs = len(pools.segs)
    graph, pipe = pipeline_of(env, pools)
    graph.steps[77_777] = (n_segs << 1) | 1  # segment id == n_segs
    torch.cuda.synchronize()
    pipe.steps_changed()
    bufs = [buffers(n_segs) for _ in range(3)]
    for k in range(4):  # the first from the steps, the others from the image
        with Profile() as prof:
            for b in bufs:
                pipe.seg_depth(*b)
            with pytest.raises(pa.FlatGFAError) as err:
                pipe.status()
        assert err.value.code == -2, k
        if k == 0:
            desc = pipe.describe()
            assert IMAGE.search(desc) and RECORDS.search(desc).group(1) == "kept", desc
        else:
            assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (3, 3, 3), (k, prof.names)
    graph.steps[77_777] = int(pools.steps[77_777])
    torch.cuda.synchronize()
    pipe.steps_changed()
    warm_round(pipe, n_segs, want)  # (... and with the step put back, the answers are back)
    pipe.close()


# ---- D. handles that own their buffers ----

def pools_of(g):
    return fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})


def widened(want):
    return want[0].astype(np.uint64), want[1].astype(np.uint64)


@pytest.mark.parametrize("parts", ["2", None, "1"])
def test_a_resident_graph_queried_again_and_again(env, parts):
    """The handle's plan and its subset plan write different answers into the handle's two buffers (capi.cpp: d_depth, d_uniq),
    call and status each time: from the third query on these are image calls, and kept calls from the one after.  With two
    workgroups per window a kept call that did not zero them would add to the other plan's answer.  With one, path_depth
    is the fused call, which overwrites the full plan's records: behind it (queries 9 to 11) the subset plan makes an image
    call and the full plan the next -- whose records are gone, whatever the other plan has kept."""
    if parts:
        env.setenv("FLATGFA_ACC_PARTS", parts)
    pools, want = synth_case(*PANGENOME)
    want = widened(want)
    g = pa.synth(*PANGENOME[:4], PANGENOME[4], False)
    assert (pools_of(g).steps == pools.steps).all()
    begins, ends = spans_of(pools)
    some = np.arange(0, len(begins), 3)
    want_sub = widened(fo.seg_depth_with_uniq(make_pools(pools.steps, begins[some], ends[some], len(pools.segs))))
    assert (want_sub[0] != want[0]).any() and (want_sub[0] != want_sub[1]).any()
    want_ln, want_mean = fo.path_depth(pools_of(g))
    g.to_device(0)

    def both(what):
        d, u = g.seg_depth_with_uniq()
        assert (d == want[0]).all() and (u == want[1]).all(), what

    def depth_only(what):
        assert (g.seg_depth() == want[0]).all(), what

    def subset(what):
        d, u = g.seg_depth_subset(some)
        assert (d == want_sub[0]).all() and (u == want_sub[1]).all(), what

    def path_depth(what):
        ln, mean = g.path_depth()
        assert (ln == want_ln).all() and mean.tobytes() == want_mean.tobytes(), what

    kept, fused = [], []
    for k, query in enumerate((both, depth_only, both, subset, both, subset, path_depth, both, path_depth, subset, both)):
        with Profile() as prof:
            query(f"query {k + 1}")
        # (query 4 makes the subset plan, whose creation launches kernels of its own: not counted)
        if 2 <= k < 8 and k != 3 and prof.pass2() and prof.pass1() < prof.pass2():
            kept.append(k + 1)
        if query is path_depth:
            fused.append(prof.count("k_accum<depth+paths>"))
    assert kept, "no query among 3 to 8 ran on kept records"
    assert fused == ([1, 1] if parts == "1" else [0, 0]), fused
    g.close()


def test_a_sharded_graph_queried_six_times(env):
    """Three shards on one device, one path cut between them: every shard's plan, and the plan of each piece of the cut path,
    calls into the shard's own buffers (sharded.hip: d_send, d_tmp) again and again."""
    rng = np.random.default_rng(3)
    S = 20_000
    lens = [200_000] + [int(x) for x in rng.integers(50, 4000, size=40)]  # one path far longer than a shard's share
    ids = [((np.arange(n) * 7 + rng.integers(0, S)) % S).astype(np.uint32) for n in lens]
    lines = [f"S\t{i + 1}\tACGT" for i in range(S)]
    for k, walk in enumerate(ids):
        lines.append(f"P\tp{k}\t" + ",".join(f"{int(x) + 1}+" for x in walk) + "\t*")
    g = pa.parse_bytes(("\n".join(lines) + "\n").encode())
    want = fo.seg_depth_with_uniq(pools_of(g))
    assert (want[0] != want[1]).any()
    kept = []
    with pa.ShardedFlatGFA(g, 3, devices=[0, 0, 0]) as sh:
        assert sh.layout()[0]["split_paths"] >= 1
        for k in range(6):
            with Profile() as prof:
                if k % 2 == 0:
                    d, u = sh.seg_depth_with_uniq()
                else:
                    d, u = sh.seg_depth(), None
            assert (d == want[0]).all(), (k, "depth", np.flatnonzero(d != want[0])[:8])
            assert u is None or (u == want[1]).all(), (k, "uniq", np.flatnonzero(u != want[1])[:8])
            if k >= 2 and prof.pass2() and prof.pass1() < prof.pass2():
                kept.append(k + 1)
    assert kept, "no query ran on kept records"


# ---- E. the default rule ----

def test_without_hooks_the_image_comes_with_the_graphs_size(monkeypatch):
    """No hook set: a plan reads the image from 2^24 steps (64 MiB of them) on, and keeps the records then; one step fewer and
    every call runs k_scan.  The benchmark's pangenome model at a sixth of its paths: a million segments, paths of a hundred
    thousand steps (none short enough for the wave-per-path kernels), 168 of them -- and the last one cut for the second half."""
    from pollen_amd.device import DepthPlan, DeviceGraph
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    n_segs, n_paths, length = 1_000_000, 168, 100_000
    assert (n_paths - 1) * length < 2 ** 24 <= n_paths * length
    g = pa.synth(7, n_segs, n_paths, length, "pangenome", False)
    steps = pools_of(g).steps
    begins = np.arange(n_paths, dtype=np.uint64) * length
    ends = begins + length
    cap = lambda text: int(re.search(r"bucket_cap=(\d+)", text).group(1))

    pools = make_pools(steps, begins, ends, n_segs)
    want = fo.seg_depth_with_uniq(pools)
    plan = DepthPlan(DeviceGraph(pools.steps, *spans_of(pools), n_segs))
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call")
    desc = plan.describe()
    assert "short_paths=0 medium_paths=0 tiny_paths=0 " in desc, desc
    assert IMAGE.search(desc) and RECORDS.search(desc) and RECORDS.search(desc).group(1) == "kept", desc
    five_calls(plan, n_segs, want)
    five_calls(plan, n_segs, want, runs=0 if cap(plan.describe()) == cap(desc) else 1)
    plan.close()

    ends[-1] -= n_paths * length - (2 ** 24 - 1)
    pools = make_pools(steps[:2 ** 24 - 1], begins, ends, n_segs)
    want = fo.seg_depth_with_uniq(pools)
    plan = DepthPlan(DeviceGraph(pools.steps, *spans_of(pools), n_segs))
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call, one step below")
    desc = plan.describe()
    assert "path=bucketed" in desc and "run_image=" not in desc, desc
    bufs = [buffers(n_segs) for _ in range(5)]
    with Profile() as prof:
        for b in bufs:
            plan.seg_depth(*b)
        plan.status()
    for k, b in enumerate(bufs):
        assert_right(b, want, f"call {k} of five, one step below")
    assert (prof.count("k_scan_runs"), prof.count("k_scan"), prof.pass1(), prof.pass2()) == (0, 5, 5, 5), prof.names
    plan.close()
