"""Pass 2 on the plan's sorted record image: the calls that run on kept records sweep the records sorted
by (window, path, start) -- revisits from a running maximum of the path's earlier ends, no bitsets -- against the C oracle, bit
for bit, in buffers pre-filled with -1, with and without unique depth.

The environment is test_gpu_kept_records.py's: FLATGFA_RUN_IMAGE=1, the bucketed path, every path an item of pass 1, no pass 1
by partition, no per-block marks; one pass-2 workgroup per window and 4096-segment windows unless a case says otherwise.  Every
case makes a plan, makes the first call (k_scan on the steps: the images are made behind it) and asks for the description, which
waits for them and says ` pass2=sorted`; then a call that runs k_scan_runs, and calls on kept records, which run the sweep (the
profile's scope names are pass 2's as ever: that it is the sweep that ran shows in the mutants the cases catch, listed in
profiles/NOTES.md R7.3).  Graphs are hand-laid id lists, a few thousand steps at the most; one case per model is synthetic.
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
         "FLATGFA_PATH_GROUPS", "FLATGFA_KEEP_RECORDS", "FLATGFA_SORTED_RECORDS")
IMAGE = re.compile(r" run_image=(\d+)\b")
PASS2 = re.compile(r" pass2=(sorted|walk\((\w+)\)) records=(kept|rewritten)$")
CHUNK = re.compile(r" sorted_chunk=(\d+) ")
W = 4096
FAR = 3500  # (ids from here up separate the runs of a hand-laid path: two runs laid one behind the other must not join)


@pytest.fixture
def env(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FLATGFA_RUN_IMAGE", "1")
    monkeypatch.setenv("FLATGFA_DEPTH_PATH", "bucketed")
    monkeypatch.setenv("FLATGFA_SHORT_MAX", "0")
    monkeypatch.setenv("FLATGFA_DENSE", "0")
    monkeypatch.setenv("FLATGFA_NO_CLAIM_BLOCKS_OFF", "1")
    monkeypatch.setenv("FLATGFA_ACC_PARTS", "1")
    monkeypatch.setenv("FLATGFA_WB", "12")
    return monkeypatch


def make_pools(steps, begins, ends, n_segs):
    base = synth.pools(1, n_segs, 1, 1)
    paths = np.zeros(len(begins), dtype=base.paths.dtype)
    paths["steps_start"] = np.asarray(begins, dtype=np.uint64)
    paths["steps_end"] = np.asarray(ends, dtype=np.uint64)
    return dataclasses.replace(base, paths=paths, steps=np.ascontiguousarray(steps, dtype=np.uint32))


def spans_of(pools):
    return pools.paths["steps_start"].astype(np.uint32), pools.paths["steps_end"].astype(np.uint32)


def laid_out(paths, lead=0):
    steps, begins, ends = [np.zeros(lead, dtype=np.uint32)], [], []
    at = lead
    for ids in paths:
        ids = np.asarray(ids, dtype=np.uint32)
        begins.append(at)
        ends.append(at + len(ids))
        steps.append(ids << 1)
        at += len(ids)
    return np.concatenate(steps), begins, ends


def runs(*spans, far=FAR):
    """One path's ids: the runs [a, b) (b < a: downwards, a-1 .. b), a lone far id between any two."""
    out = []
    for k, (a, b) in enumerate(spans):
        if k:
            out.append(np.array([far + 2 * k]))
        out.append(np.arange(a, b) if b >= a else np.arange(a - 1, b - 1, -1))
    return np.concatenate(out)


def graph_of(paths, n_segs, lead=0):
    steps, b, e = laid_out(paths, lead)
    pools = make_pools(steps, b, e, n_segs)
    return pools, fo.seg_depth_with_uniq(pools)


def buffers(n_segs, uniq=True):
    import torch
    d = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")
    return d, (torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0") if uniq else None)


def assert_right(bufs, want, what):
    d, u = bufs
    got = d.cpu().numpy().view(np.uint32)
    assert (got == want[0]).all(), (what, "depth", np.flatnonzero(got != want[0])[:8], got[got != want[0]][:8], want[0][got != want[0]][:8])
    if u is not None:
        got = u.cpu().numpy().view(np.uint32)
        assert (got == want[1]).all(), (what, "uniq", np.flatnonzero(got != want[1])[:8], got[got != want[1]][:8], want[1][got != want[1]][:8])


class Profile:
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


def plan_of(pools, seg_len=False):
    from pollen_amd.device import DepthPlan, DeviceGraph
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    lens = np.ascontiguousarray(pools.seg_lens(), dtype=np.uint32) if seg_len else None
    graph = DeviceGraph(pools.steps, begins, ends, n_segs, lens)
    return graph, DepthPlan(graph), n_segs


def first_call(plan, n_segs, want, expect="sorted"):
    """The first call (k_scan on the steps), checked, and the description once the images are there: which pass 2 it names."""
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call")
    desc = plan.describe()
    assert IMAGE.search(desc), desc
    m = PASS2.search(desc)
    assert m and (m.group(1) == expect) and m.group(3) == "kept", desc
    return desc


def sorted_calls(plan, n_segs, want, scans=1):
    """A call that runs pass 1 from the run image, then three on kept records: with unique depth, without, with -- one k_scan_runs, four pass 2."""
    bufs = [buffers(n_segs), buffers(n_segs), buffers(n_segs, uniq=False), buffers(n_segs)]
    with Profile() as prof:
        for b in bufs:
            plan.seg_depth(*b)
        plan.status()
    for k, b in enumerate(bufs):
        assert_right(b, want, f"call {k} behind the first")
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (scans, scans, 4), prof.names
    assert (prof.count("k_accum<uniq>"), prof.count("k_accum<depth>")) == (3, 1), prof.names


def check(pools, want, expect="sorted"):
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want, expect)
    sorted_calls(plan, n_segs, want)
    plan.close()
    return desc


# ---- the sweep: one path's records in one window ----

SWEEP = {
    "nested": [runs((100, 300), (150, 200))],
    "identical": [runs((100, 200), (100, 200))],
    "abutting": [runs((100, 150), (150, 200))],  # e == the next s: no revisit
    "one_cell": [runs((100, 150), (149, 200))],
    "same_start": [runs((100, 150), (100, 130), (100, 180))],
    "up_and_down": [np.concatenate([np.arange(100, 200), np.arange(199, 99, -1), np.arange(100, 200)])],
    "1_2_5_and_another": [runs((10, 11), (20, 21), (30, 31), (20, 21), (30, 31), (30, 31), (30, 31), (30, 31)), runs((10, 11), (20, 21), (30, 31))],
    "window_end": [runs((4090, 4096), (4000, 4096), (4095, 4096), far=2000)],  # records ending on the window's last cell
}


@pytest.mark.parametrize("case", sorted(SWEEP))
def test_the_sweep_counts_a_paths_revisits(env, case):
    pools, want = graph_of(SWEEP[case], 9_000)  # (not a multiple of the window: the last one is partial)
    assert (want[0] != want[1]).any() or case == "abutting"
    if case == "abutting":
        assert (want[0][100:200] == 1).all() and (want[1][100:200] == 1).all()
    if case == "1_2_5_and_another":
        assert list(want[0][[10, 20, 30]]) == [2, 3, 6] and list(want[1][[10, 20, 30]]) == [2, 2, 2]
    check(pools, want)


# ---- path seams inside a chunk ----

def test_hundreds_of_paths_with_a_few_records_each(env):
    rng = np.random.default_rng(5)
    paths = []
    for p in range(400):
        spans = []
        for _ in range(1 + p % 3):
            a = int(rng.integers(0, 3400))
            spans.append((a, a + int(rng.integers(1, 9))))
        paths.append(runs(*spans, far=3450 + (p % 40)))
    paths.append(paths[7].copy())  # the same ids in another span: another path
    pools, want = graph_of(paths, 9_000, lead=3)
    only = np.setdiff1d(paths[7][paths[7] < 3400], np.concatenate([q[q < 3400] for k, q in enumerate(paths[:-1]) if k != 7]))
    if len(only):
        assert (want[1][only] == 2).all()
    check(pools, want)


def test_two_paths_over_the_same_ids_count_twice(env):
    ids = runs((50, 90), (60, 70), (4000, 4200))
    pools, want = graph_of([ids, ids.copy()], 9_000)
    assert (want[1][50:90] == 2).all() and (want[0][60:70] == 4).all()
    check(pools, want)


# ---- chunk seams and the carry ----

def chunk_of(desc):
    return int(CHUNK.search(desc).group(1))


@pytest.mark.parametrize("n", [62, 63, 64, 65, 127, 128, 129])
def test_a_long_run_and_short_runs_inside_it_across_chunks(env, n):
    """One path: a run of 1000 segments from the window's start (its first record in the order), then n short runs inside it
    (two segments apart: they never join) -- every one a revisit, in a later chunk only by the chunk's carry word -- for n
    around C and 2 C, C = 64 records per chunk as built.  The path has n + 1 records; the second path's lie behind them, inside
    the same 1000 segments, and for n = C - 1 and 2 C - 1 begin on a chunk's first lane: their carry is 0, their segments are
    first visits."""
    first = np.concatenate([np.arange(0, 1000)] + [np.arange(3 + 5 * i, 6 + 5 * i) for i in range(n)])
    second = np.concatenate([np.arange(500, 520), np.arange(400, 420), np.arange(410, 415)])
    pools, want = graph_of([first, second], 9_000)
    assert (want[1][:1000] >= 1).all() and want[1][:400].max() == 1 and (want[1][410:415] == 2).all()
    desc = check(pools, want)
    assert chunk_of(desc) == 64, "the cases are laid out for chunks of 64 records"


def test_windows_with_exactly_a_chunk_one_record_and_none(env):
    c_runs = np.concatenate([np.arange(3 * i, 3 * i + 2) for i in range(64)])  # 64 records in window 0, nothing else there
    one = np.arange(2 * W + 100, 2 * W + 140)                                  # one record in window 2; window 1 has none
    pools, want = graph_of([c_runs, one], 3 * W + 17)
    assert want[0][W:2 * W].max() == 0
    check(pools, want)


# ---- windows ----

@pytest.mark.parametrize("wb", [11, 12, 13])
def test_runs_split_at_window_edges_at_every_width(env, wb):
    env.setenv("FLATGFA_WB", str(wb))
    w = 1 << wb
    paths = [np.concatenate([np.arange(w - 100, w + 100), np.arange(2 * w + 50, 2 * w - 50, -1), np.arange(w - 10, w + 10), np.arange(w - 3, w)]),
             np.concatenate([np.arange(w + 60, w - 60, -1), np.arange(w - 1, w + 1), np.arange(3 * w - 40, 3 * w + 30)])]
    pools, want = graph_of(paths, 3 * w + 30)  # (the last window holds 30 segments)
    desc = check(pools, want)
    assert f"x{w} " in desc, desc


# ---- split paths ----

def test_the_pieces_of_a_split_path_sort_as_one_path(env):
    env.setenv("FLATGFA_PIECE_STEPS", "700")
    paths = [np.concatenate([np.arange(0, 3000), np.arange(2000, 5000), np.arange(2990, 3010)]), np.arange(8500, 500, -1)]
    pools, want = graph_of(paths, 9_000, lead=7)
    _, plan, n_segs = plan_of(pools)
    desc = first_call(plan, n_segs, want)
    assert int(re.search(r"split_paths=(\d+)", desc).group(1)) > 0, desc
    sorted_calls(plan, n_segs, want)
    plan.close()


# ---- state ----

def test_other_calls_between_sorted_calls(env):
    """A path-depth call writes other records into the scratch: right, and the call behind it runs pass 1 again.  A depth-only
    call shares the kept records, as it always has: right, and no pass 1 behind it."""
    import torch
    from pollen_amd.device import DepthPlan, DeviceGraph
    pools, want = synth_case("pangenome", 9_000, 30, 5_000)
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    seg_len = np.ascontiguousarray(pools.seg_lens(), dtype=np.uint32)
    plan = DepthPlan(DeviceGraph(pools.steps, begins, ends, n_segs, seg_len))
    first_call(plan, n_segs, want)
    a, b, c, e, f = buffers(n_segs), buffers(n_segs), buffers(n_segs, uniq=False), buffers(n_segs), buffers(n_segs)
    d = torch.full((n_segs,), -1, dtype=torch.int32, device="cuda:0")
    ln = torch.full((len(begins),), -1, dtype=torch.int64, device="cuda:0")
    ws = torch.full((len(begins),), -1, dtype=torch.int64, device="cuda:0")
    with Profile() as prof:
        plan.seg_depth(*a)   # k_scan_runs
        plan.seg_depth(*b)   # sorted
        plan.seg_depth(*c)   # sorted, depth only
        plan.path_depth_all(d, ln, ws)
        plan.seg_depth(*e)   # k_scan_runs again
        plan.seg_depth(*f)   # sorted
        plan.status()
    for k, x in enumerate((a, b, c, e, f)):
        assert_right(x, want, k)
    assert_right((d, None), want, "path_depth_all's depth")
    assert (prof.count("k_scan_runs"), prof.count("k_scan")) == (2, 1), prof.names
    plan.close()


def test_an_id_out_of_range_keeps_the_walk_and_the_error(env):
    """A record dropped for bounds: the sorted image is not installed (pass 1 has an error to raise), and every round raises it.
    This is the one status error there is to test around the sweep: k_accum_sorted raises no status bit and reads no bucket, so
    once ` pass2=sorted` is installed an error can only come from a call that runs pass 1, and a plan whose pass 1 has one to
    raise never gets the image.  "A status that reads an error BETWEEN sorted calls" is therefore not reachable; what a status
    that reads anything does to the kept records is test_gpu_kept_records.py's, unchanged."""
    import torch
    pools, _ = synth_case("pangenome", 9_000, 8, 5_000)
    graph, plan, n_segs = plan_of(pools)
    d, u = buffers(n_segs)
    graph.steps[7_777] = (n_segs << 1) | 1
    torch.cuda.synchronize()
    plan.steps_changed()
    for k in range(4):
        with Profile() as prof:
            plan.seg_depth(d, u)
            with pytest.raises(pa.FlatGFAError) as err:
                plan.status()
        assert err.value.code == -2, k
        if k == 0:
            desc = plan.describe()
            m = PASS2.search(desc)
            assert m and m.group(2) == "bounds", desc
        else:
            assert prof.count("k_scan_runs") == 1, (k, prof.names)
    graph.steps[7_777] = int(pools.steps[7_777])
    plan.close()


def test_steps_changed_makes_the_image_again(env):
    import torch
    pools, want = synth_case("pangenome", 9_000, 8, 5_000)
    graph, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    sorted_calls(plan, n_segs, want)
    changed = pools.steps.copy()
    at = np.arange(100, 39_000, 97)
    changed[at] = ((changed[at] >> 1 ^ 4097) % n_segs << 1).astype(np.uint32)
    graph.steps[torch.from_numpy(at).to("cuda:0")] = torch.from_numpy(changed[at].view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    plan.steps_changed()
    want2 = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
    assert (want2[0] != want[0]).any() and (want2[1] != want[1]).any()
    first_call(plan, n_segs, want2)  # (a stale image would give the old answer from the third call on)
    sorted_calls(plan, n_segs, want2)
    plan.close()


def test_three_lanes_six_calls_in_flight(env):
    from pollen_amd.device import DepthPipeline, DeviceGraph
    pools, want = synth_case("chromosome", 20_000, 24, 5_000)
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
    m = PASS2.search(desc)
    assert IMAGE.search(desc) and m and m.group(1) == "sorted", desc
    assert " sorted_image_plans=3 " in desc, desc  # (the lanes have the same paths and windows: one image for the three)
    for _ in range(2):
        bufs = [buffers(n_segs, uniq=k != 4) for k in range(6)]
        with Profile() as prof:
            for b in bufs:
                pipe.seg_depth(*b)
            pipe.status()
        for k, b in enumerate(bufs):
            assert_right(b, want, k)
    # (the second six: every lane's records are kept, unless the status between found a sub-bucket more than half full and a lane's buckets grew)
    assert prof.pass1() <= 3 and prof.pass2() == 6 and prof.count("k_scan") == 0, prof.names
    pipe.close()


def test_plans_over_the_same_paths_share_an_image_and_others_do_not(env):
    """Two plans of one graph hold one sorted image (made of the first one's items); a plan over every third path of the same step
    array has other records and an image of its own.  Closing the plan that made the shared image leaves it to the other."""
    from pollen_amd.device import DepthPlan, DeviceGraph
    pools, want = synth_case("pangenome", 9_000, 30, 5_000)
    n_segs = len(pools.segs)
    begins, ends = spans_of(pools)
    graph = DeviceGraph(pools.steps, begins, ends, n_segs)
    some = np.arange(0, len(begins), 3)
    sub = DeviceGraph.from_tensors(graph.steps, graph.path_begin[::3].contiguous(), graph.path_end[::3].contiguous(), n_segs)
    want_sub = fo.seg_depth_with_uniq(make_pools(pools.steps, begins[some], ends[some], n_segs))
    assert (want_sub[1] != want[1]).any()
    first, second, third = DepthPlan(graph), DepthPlan(graph), DepthPlan(sub)
    first_call(first, n_segs, want)
    desc = first_call(second, n_segs, want)
    assert " sorted_image_plans=2 " in desc and "run_image_plans=2" in desc, desc
    desc = first_call(third, n_segs, want_sub)
    assert " sorted_image_plans=1 " in desc and "run_image_plans=3" in desc, desc
    for plan, w in ((first, want), (second, want), (third, want_sub)):
        sorted_calls(plan, n_segs, w)
    first.close()
    assert " sorted_image_plans=1 " in second.describe()
    b = buffers(n_segs)
    second.seg_depth(*b)
    second.status()
    assert_right(b, want, "behind the close of the plan that made the image")
    b = buffers(n_segs)
    third.seg_depth(*b)
    third.status()
    assert_right(b, want_sub, "the plan with an image of its own")
    second.close()
    third.close()


def test_two_workgroups_per_window_keep_the_walk(env):
    env.setenv("FLATGFA_ACC_PARTS", "2")
    pools, want = synth_case("pangenome", 9_000, 30, 5_000)
    desc = check(pools, want, expect="walk(parts)")
    assert "workgroups_per_window=2" in desc, desc


def test_with_the_hook_off_the_description_and_the_answers_are_the_walks(env):
    pools, want = synth_case("pangenome", 9_000, 30, 5_000)
    outs = {}
    for hook in ("0", None):
        if hook is None:
            env.delenv("FLATGFA_SORTED_RECORDS")
        else:
            env.setenv("FLATGFA_SORTED_RECORDS", hook)
        _, plan, n_segs = plan_of(pools)
        b = buffers(n_segs)
        plan.seg_depth(*b)
        plan.status()
        desc = plan.describe()
        if hook == "0":
            assert " pass2=sorted" not in desc and " pass2=walk" not in desc and "sorted_" not in desc and desc.endswith(" records=kept"), desc
            off = desc
        else:
            assert re.sub(r" sorted_image=\d+ sorted_image_build=\d+ sorted_image_plans=1 sorted_chunk=\d+ pass2=sorted", "", desc) == off, (desc, off)
        bufs = [buffers(n_segs) for _ in range(3)]
        for x in bufs:
            plan.seg_depth(*x)
        plan.status()
        outs[hook] = [(x[0].cpu().numpy(), x[1].cpu().numpy()) for x in bufs]
        plan.close()
    for (d0, u0), (d1, u1) in zip(outs["0"], outs[None]):
        assert (d0 == d1).all() and (u0 == u1).all()
        assert (d0.view(np.uint32) == want[0]).all() and (u0.view(np.uint32) == want[1]).all()


# ---- ordinary data through every stage ----

_WANT = {}


def synth_case(model, n_segs, n_paths, length, seed=7):
    key = (seed, n_segs, n_paths, length, model)
    if key not in _WANT:
        pools = synth.pools(seed, n_segs, n_paths, length, model)
        _WANT[key] = (pools, fo.seg_depth_with_uniq(pools))
    return _WANT[key]


@pytest.mark.parametrize("model", ["pangenome", "chromosome"])
def test_a_synthetic_graph_through_every_stage(env, model):
    pools, want = synth_case(model, 65_536, 100, 5_000)
    if model == "pangenome":
        assert (want[0] != want[1]).any()
    check(pools, want)
