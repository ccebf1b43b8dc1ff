"""The sweep over the sorted record image in groups of four chunks: a lane of k_accum_sorted holds four
consecutive records, a record's path ordinal comes out of the image, a chunk's carry word is a seed in the group's one scan, and
only the group with a window's last chunk looks for padding.  Hand-laid paths on at most three windows, laid so that records fall
on the seams of that scheme -- a lane's four, a chunk inside a group, a group, a window's tail of one to four chunks -- against
the C oracle, bit for bit, in buffers pre-filled with -1.

The environment and the helpers are test_gpu_sorted_records.py's.  Every case makes a plan and its first call, asks for the
description (which waits for the images) and asserts ` pass2=sorted`; makes the one call that runs k_scan_runs; and then profiles
calls on kept records, with unique depth and without, which must run one pass 2 each and no k_scan*.  The library's profile
names scopes, not kernels -- pass 2's scope is `k_accum<...>` whichever kernel it launches -- so that it is k_accum_sorted that
ran is what the description says and what the mutants of profiles/NOTES.md R7.4 show: each of them changes the sweep or the
image alone and fails cases here.  No case passes through the walk.

Where a case needs a window of exactly N records, `records_per_window` -- a model of how the plan cuts paths into records (a run
of ids going up by one, cut at path ends, at every 1024th step of the step array and at window edges) -- counts them, and the
case asserts the count before it runs.  An accumulating call (FastPlan::accumulate: a group of paths behind the first) is not
among the cases: plans with more than one group of paths get no image (`walk(ranges)`), so no call reaches the sweep with it.
"""
import collections

import numpy as np
import pytest

from oracle import flatgfa_oracle as fo
from test_gpu_sorted_records import IMAGE, PASS2, Profile, assert_right, buffers, env, first_call, graph_of, plan_of, spans_of  # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu

W = 4096


@pytest.fixture
def genv(env):
    env.setenv("FLATGFA_PIECE_STEPS", str(1 << 20))  # (no path here is cut into pieces: a cut would split a run into two records)
    return env


def records_per_window(paths, wb=12, lead=0):
    """How many records every window gets.  The layouts here jump by two ids or more between runs and never turn round, so a run
    is a stretch of ids going up by one; the model refuses anything else."""
    out = collections.Counter()
    pos = lead
    for ids in paths:
        ids = np.asarray(ids, dtype=np.int64)
        step = np.diff(ids)
        assert not (step == -1).any(), "the model knows runs that go up only"
        cut = np.flatnonzero((step != 1) | ((pos + 1 + np.arange(len(step))) % 1024 == 0)) + 1
        for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(ids)]])):
            for w in range(int(ids[a]) >> wb, (int(ids[b - 1]) >> wb) + 1):
                out[w] += 1
        pos += len(ids)
    return out


def shorts(n, base=0, stride=3, length=2):
    """n runs of `length` ids, `stride` apart (two ids or more between them: they never join)."""
    assert stride >= length + 1
    return np.concatenate([np.arange(base + stride * i, base + stride * i + length) for i in range(n)]) if n else np.zeros(0, dtype=np.int64)


def sweep_calls(plan, n_segs, want):
    """The call that runs k_scan_runs, then three on kept records under the profile: one pass 2 each, no pass 1 of any kind."""
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "the call that runs k_scan_runs")
    bufs = [buffers(n_segs), buffers(n_segs, uniq=False), buffers(n_segs)]
    with Profile() as prof:
        for x in bufs:
            plan.seg_depth(*x)
        plan.status()
    assert (prof.pass1(), prof.pass2()) == (0, 3), prof.names
    assert (prof.count("k_accum<uniq>"), prof.count("k_accum<depth>")) == (2, 1), prof.names
    for k, x in enumerate(bufs):
        assert_right(x, want, f"sweep {k}")


def check(paths, n_segs, lead=0):
    pools, want = graph_of(paths, n_segs, lead)
    _, plan, n = plan_of(pools)
    desc = first_call(plan, n, want)  # (asserts ` pass2=sorted records=kept`)
    sweep_calls(plan, n, want)
    plan.close()
    return desc, want


# ---- windows of every tail: one to four chunks in the last group, full and not ----

def window_of(n, base, other_path=True, pos=0):
    """Paths, laid into the step array from position `pos` on, that put exactly n records into the window that begins at `base`:
    one path's run of 900 and short runs, most of them inside it; another path's short runs over the same ids (first visits:
    another path), one of them twice."""
    if n == 0:
        return []
    b = (n - 1) // 3 if other_path else 0
    for a in range(n - 1 - b, max(n - 5 - b, -1), -1):  # (a cut of the step array inside a run makes one record more)
        paths = [np.concatenate([np.arange(base, base + 900), shorts(a, base + 1)])]
        if b:
            paths.append(shorts(b, base) if b < 4 else np.concatenate([shorts(b - 1, base), np.arange(base, base + 2)]))
        if records_per_window(paths, lead=pos)[base >> 12] == n:
            return paths
    raise AssertionError((n, base, pos))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 255, 256, 257, 511, 512, 513, 1025])
def test_a_window_of_n_records_an_empty_one_and_another(genv, n):
    """Window 0 has n records -- a tail group of one, two or three chunks; a chunk count that is a multiple of four with a partly
    filled last chunk (200) and a full one (256, 512); one chunk more than that --, window 1 none, window 2 seventy."""
    paths = window_of(n, 0)
    paths += window_of(70, 2 * W, other_path=False, pos=sum(len(p) for p in paths))
    got = records_per_window(paths)
    assert (got[0], got[1], got[2]) == (n, 0, 70), got
    _, want = check(paths, 3 * W + 17)
    assert want[0][W:2 * W].max() == 0
    if n >= 65:
        assert (want[0][:900] > want[1][:900]).any()  # (revisits behind the first chunk)


# ---- one path's long run and short runs inside it: a revisit found across a lane's edge, a chunk's, a group's ----

def long_and_shorts(total):
    """One path of `total` records in window 0: a run of 1000 from the window's start, its first record in the order, and short
    runs inside it, every one a revisit."""
    for n in range(max(total - 8, 0), total):
        ids = np.concatenate([np.arange(0, 1000), shorts(n, 1)])
        if records_per_window([ids])[0] == total:
            assert 3 * n + 2 < 1000
            return ids
    raise AssertionError(total)


@pytest.mark.parametrize("total", [4, 5, 16, 17, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 320])
def test_a_long_run_and_short_runs_inside_it_across_lanes_chunks_and_groups(genv, total):
    """The record at position k of the order (k = 1 .. total - 1) is a revisit by the long run at position 0 alone: inside its
    lane for k < 4, by the scan across lanes inside chunk 0, by chunk 1..3's seed inside group 0, and in a later group by its
    chunk's carry word and nothing else."""
    first = long_and_shorts(total)
    _, want = check([first], 2 * W + 9)
    n = total - 1
    assert (want[0][:1000] >= 1).all() and (want[1][:1000] == 1).all() and want[0][:1000].max() == 2 and int((want[0][:1000] == 2).sum()) >= 2 * (n - 1)


@pytest.mark.parametrize("total", [64, 128, 192, 256, 320])
def test_a_second_path_that_begins_on_a_chunks_first_record(genv, total):
    """... with a second path behind it whose first record is the first of chunk 1, 2 or 3 of group 0 (64, 128, 192), of group 1
    (256) and of chunk 1 of group 1 (320): its carry is 0, its ordinal starts again at 1, and its segments, which lie inside the
    first path's long run, are first visits -- but for the five it walks twice."""
    first = long_and_shorts(total)
    second = np.concatenate([np.arange(500, 520), np.arange(400, 420), np.arange(410, 415)])
    assert records_per_window([first, second])[0] == total + 3
    _, want = check([first, second], 2 * W + 9)
    assert (want[1][410:415] == 2).all() and want[1][:400].max() == 1 and (want[1][500:520] == 2).all() and (want[0][410:415] >= 3).all()


# ---- every record a first: the ordinal reaches 64 ----

@pytest.mark.parametrize("n_paths", [64, 65, 256, 257])
def test_paths_of_a_single_record_fill_a_chunk_and_a_group(genv, n_paths):
    paths = [np.arange(5 * i, 5 * i + 8) for i in range(n_paths)]  # (neighbours overlap by three ids: another path's, no revisit)
    assert records_per_window(paths)[0] == n_paths
    _, want = check(paths, W + 100)
    assert (want[0] == want[1]).all() and want[0][:5 * n_paths].max() == 2


# ---- two paths over the same ids ----

def test_two_paths_interleaved_by_start_and_records_with_equal_starts(genv):
    a = np.concatenate([np.arange(10 * i, 10 * i + 7) for i in range(0, 80, 2)] + [np.arange(100, 150), np.arange(100, 130), np.arange(100, 180), np.arange(96, 140)])
    b = np.concatenate([np.arange(10 * i, 10 * i + 7) for i in range(1, 80, 2)] + [np.arange(100, 130), np.arange(100, 180), np.arange(100, 101), np.arange(3, 300)])
    _, want = check([a, b, a.copy(), b.copy()], 2 * W)
    assert (want[1][100:130] == 4).all() and (want[0][100:130] >= 12).all()


# ---- window edges at every width ----

@pytest.mark.parametrize("wb", [11, 12, 13])
def test_runs_across_window_edges_at_every_width(genv, wb):
    """Runs that cross a window's edge become two records; one ends on window 0's last cell (its end lands in the sink cell); the
    last window holds 30 segments.  Both full windows get more than a group of records."""
    genv.setenv("FLATGFA_WB", str(wb))
    w = 1 << wb
    paths = [np.concatenate([np.arange(w - 100, w + 100), np.arange(2 * w - 50, 2 * w + 30), np.arange(w - 10, w + 10), np.arange(w - 3, w), np.arange(w - 700, w),
                             shorts(300, w - 950), shorts(140, w + 2), np.arange(w - 1, w + 1)]),
             np.concatenate([np.arange(w - 60, w + 60), np.arange(w - 1, w + 1), np.arange(2 * w - 40, 2 * w + 30), shorts(90, w - 200), np.arange(w - 1, w)])]
    got = records_per_window(paths, wb)
    assert got[0] > 256 and got[1] > 128 and 0 < got[2] < 64, got
    desc, want = check(paths, 2 * w + 30)
    assert f"x{w} " in desc, desc
    assert want[0][w - 1] > want[1][w - 1] and want[0][2 * w + 29] == 2


# ---- call kinds ----

def test_three_lanes_share_one_image(genv):
    from pollen_amd.device import DepthPipeline, DeviceGraph
    paths = window_of(300, 0) + window_of(513, W) + [long_and_shorts(258) + 2 * W]
    pools, want = graph_of(paths, 3 * W)
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
    assert " sorted_image_plans=3 " in desc, desc
    for _ in range(2):
        bufs = [buffers(n_segs, uniq=k != 4) for k in range(6)]
        with Profile() as prof:
            for b in bufs:
                pipe.seg_depth(*b)
            pipe.status()
        for k, b in enumerate(bufs):
            assert_right(b, want, k)
    assert prof.pass1() == 0 and prof.pass2() == 6, prof.names  # (the second six: every lane's records are kept)
    pipe.close()


def test_steps_changed_makes_the_image_and_its_ordinals_again(genv):
    """Other ids through the same two path spans behind steps_changed(): the first path's 101 records become 300, the second's
    300 become 101 -- every first-of-path position, ordinal and carry word of the old image is wrong for the new records."""
    import dataclasses
    import torch
    old = [np.concatenate([np.arange(0, 400), shorts(100, 1)]), shorts(300, 0)]
    new = [shorts(300, 0), np.concatenate([np.arange(200, 600), shorts(100, 201)])]
    assert [len(p) for p in old] == [len(p) for p in new] == [600, 600]
    pools, want = graph_of(old, W + 100)
    graph, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want)
    sweep_calls(plan, n_segs, want)
    changed = (np.concatenate(new) << 1).astype(np.uint32)
    graph.steps[:] = torch.from_numpy(changed.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    plan.steps_changed()
    want2 = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
    assert (want2[0] != want[0]).any() and (want2[1] != want2[0]).any()
    first_call(plan, n_segs, want2)
    sweep_calls(plan, n_segs, want2)
    plan.close()
