"""The packed cells of the sweep over the sorted record image: with unique depth a cell of k_accum_sorted
holds the depth difference in its low half and the revisit difference in its high half, a record is two LDS adds and a third only
where its revisits end before it does, and the image's build says whether the plan may sweep that way (fewer than 2^14 records
start, and fewer end, at any one cell of any window).  Hand-laid paths against the C oracle, bit for bit, in buffers pre-filled
with -1; the environment and the helpers are test_gpu_sorted_records.py's and test_gpu_sorted_groups.py's.

The description names the cells only under the hook that forces one form (`FLATGFA_SORTED_CELLS=wide|packed`), at the line's end:
` sorted_cells=packed`, ` sorted_cells=wide(hook)`, ` sorted_cells=wide(rule)`, and behind it ` sorted_lanes=solo` or ` sorted_lanes=shared` (`FLATGFA_SORTED_SOLO=0|1`: a pipeline lane's
sweep launched one workgroup to a CU).  `packed` never overrides the rule, so a case that
sets it and reads `packed` has run the packed build, and one that reads `wide(rule)` the wide one.
"""
import dataclasses
import re

import numpy as np
import pytest

from oracle import flatgfa_oracle as fo
from test_gpu_sorted_groups import genv, long_and_shorts, records_per_window, shorts, sweep_calls, window_of  # noqa: F401 (genv is a fixture)
from test_gpu_sorted_records import IMAGE, Profile, assert_right, buffers, env, graph_of, plan_of, spans_of  # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu

W = 4096
CELLS = re.compile(r" pass2=sorted records=kept sorted_cells=(packed|wide\((\w+)\)) sorted_lanes=(solo|shared)$")


def first_call(plan, n_segs, want, says):
    """The first call (k_scan on the steps), checked, and the description once the image is there: which cells it names."""
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call")
    desc = plan.describe()
    m = CELLS.search(desc)
    assert IMAGE.search(desc) and m and m.group(1) == says, (says, desc)
    return desc


def outputs(plan, n_segs):
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    return b[0].cpu().numpy().copy(), b[1].cpu().numpy().copy()


def plain_calls(plan, n_segs, want, rounds=6):
    """Calls with unique depth and without, checked one by one.  For windows of tens of thousands of records, where the plan may
    make its sub-buckets larger between two calls and run pass 1 once more: sweep_calls' count of the launches does not hold."""
    for k in range(rounds):
        b = buffers(n_segs, uniq=k != 3)
        plan.seg_depth(*b)
        plan.status()
        assert_right(b, want, f"call {k} behind the first")


def check(genv, paths, n_segs, cells="packed", says="packed", calls=sweep_calls):
    genv.setenv("FLATGFA_SORTED_CELLS", cells)
    pools, want = graph_of(paths, n_segs)
    _, plan, n = plan_of(pools)
    first_call(plan, n, want, says)
    calls(plan, n, want)
    plan.close()
    return want


def chain(n, revisiting, base=10, length=5):
    """One path of n runs with rising starts, so the order of the image is the order here and a lane holds records 4L .. 4L+3:
    of every four, the first `revisiting` start three cells inside the run before them (their revisits end at that run's end, before
    their own: the third add), the others two cells behind it.  No run's first id is next to the last id of the run before."""
    out, end = [], base
    for i in range(n):
        s = end - 3 if i and i % 4 < revisiting else end + 2
        out.append(np.arange(s, s + length))
        end = s + length
    assert end - base < 2800
    return np.concatenate(out)


# ---- windows of every tail, both builds of a group ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_a_window_of_n_records_in_packed_cells(genv, n):
    paths = window_of(n, 0)
    paths += window_of(70, 2 * W, other_path=False, pos=sum(len(p) for p in paths))
    got = records_per_window(paths)
    assert (got[0], got[1], got[2]) == (n, 0, 70), got
    want = check(genv, paths, 3 * W + 17)
    assert want[0][W:2 * W].max() == 0


# ---- revisits that end with the record (two adds) and before it (three) ----

@pytest.mark.parametrize("total", [5, 65, 257, 320])
def test_revisits_that_end_with_their_record(genv, total):
    """Short runs inside one long run: every one a revisit whose end is its own."""
    want = check(genv, [long_and_shorts(total)], 2 * W + 9)
    assert want[0][:1000].max() == 2 and (want[1][:1000] == 1).all()


@pytest.mark.parametrize("revisiting", [2, 3, 4])
@pytest.mark.parametrize("n", [9, 300])
def test_a_lane_with_two_three_and_four_records_whose_revisits_end_early(genv, n, revisiting):
    """... across a lane's seam, a chunk's (64) and a group's (256) at 300 records."""
    ids = chain(n, revisiting)
    want = check(genv, [ids, ids[: len(ids) // 2].copy()], W + 50)
    assert (want[0] > want[1]).sum() >= 2 * sum(1 for i in range(1, n) if i % 4 < revisiting)


def test_more_records_end_at_a_cell_than_start_there_under_revisits(genv):
    """Cell 900: seven runs of one path end there, all of them revisits that end with their record, one run starts there, and the
    long run they lie in goes on -- the low half of the cell goes negative under a high half that is negative too; at 893 .. 899
    the low half and the high half rise together; a second path makes the low half differ from the high one."""
    first = np.concatenate([np.arange(880, 1000), np.arange(900, 950)] + [np.arange(900 - k, 900) for k in range(7, 0, -1)] + [np.arange(850, 900)])
    second = np.concatenate([np.arange(890, 900), np.arange(895, 900), np.arange(700, 720)])
    want = check(genv, [first, second], W + 3)
    assert want[0][899] - want[0][900] >= 7 and want[0][899] > want[1][899] and want[1][899] == 2


# ---- window edges at every width: a run that ends on the window's last cell lands in the sink ----

@pytest.mark.parametrize("wb", [11, 12, 13])
def test_runs_across_window_edges_at_every_width_in_packed_cells(genv, wb):
    genv.setenv("FLATGFA_WB", str(wb))
    w = 1 << wb
    paths = [np.concatenate([np.arange(w - 100, w + 100), np.arange(2 * w - 50, 2 * w + 30), np.arange(w - 10, w + 10), np.arange(w - 3, w), np.arange(w - 700, w),
                             shorts(300, w - 950), shorts(140, w + 2), np.arange(w - 1, w + 1)]),
             np.concatenate([np.arange(w - 60, w + 60), np.arange(w - 1, w + 1), np.arange(2 * w - 40, 2 * w + 30), shorts(90, w - 200), np.arange(w - 1, w)])]
    got = records_per_window(paths, wb)
    assert got[0] > 256 and got[1] > 128 and 0 < got[2] < 64, got
    want = check(genv, paths, 2 * w + 30)
    assert want[0][w - 1] > want[1][w - 1] and want[0][2 * w + 29] == 2


# ---- the rule ----

def to_and_fro(n, a=7, b=3000):
    ids = np.empty(2 * n, dtype=np.int64)
    ids[0::2], ids[1::2] = a, b
    return ids


@pytest.mark.parametrize("n, says", [((1 << 14) - 1, "packed"), (1 << 14, "wide(rule)")])
def test_one_path_to_and_fro_between_two_cells_at_the_rules_edge(genv, n, says):
    """2n steps, n records that start at each of two cells and n that end behind each: packed with 2^14 - 1, and with 2^14 the
    plan says why not, sweeps wide cells, and agrees as well."""
    want = check(genv, [to_and_fro(n), np.arange(0, 20)], W + 10, says=says, calls=plain_calls)
    assert want[0][7] == n + 1 and want[1][7] == 2 and want[0][3000] == n and want[1][3000] == 1


def test_wide_and_packed_cells_give_the_same_vectors(genv):
    paths = [chain(300, 3), long_and_shorts(257) + W, chain(120, 4, base=W + 1200)]
    pools, want = graph_of(paths, 2 * W + 40)
    got = {}
    for cells, says in (("wide", "wide(hook)"), ("packed", "packed")):
        genv.setenv("FLATGFA_SORTED_CELLS", cells)
        _, plan, n = plan_of(pools)
        first_call(plan, n, want, says)
        outputs(plan, n)  # (the call that runs k_scan_runs)
        got[cells] = outputs(plan, n)
        plan.close()
    for k in (0, 1):
        assert (got["wide"][k] == got["packed"][k]).all() and (got["packed"][k].view(np.uint32) == want[k]).all()


def test_steps_changed_makes_the_bound_again(genv):
    """Other ids through the same path span behind steps_changed(): a rising run of 2^15 ids becomes 2^14 trips to and fro, and the
    image made again must say that its cells no longer fit -- then back."""
    import torch
    genv.setenv("FLATGFA_SORTED_CELLS", "packed")
    n = 1 << 14
    rising, fro = np.arange(0, 2 * n), to_and_fro(n)
    pools, want = graph_of([rising], 2 * n + 5)
    graph, plan, n_segs = plan_of(pools)
    first_call(plan, n_segs, want, "packed")
    plain_calls(plan, n_segs, want)
    for ids, says in ((fro, "wide(rule)"), (rising, "packed")):
        changed = (ids << 1).astype(np.uint32)
        graph.steps[:] = torch.from_numpy(changed.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        plan.steps_changed()
        want2 = fo.seg_depth_with_uniq(dataclasses.replace(pools, steps=changed))
        first_call(plan, n_segs, want2, says)
        plain_calls(plan, n_segs, want2)
    plan.close()


# ---- the builds that read past the caches ----

@pytest.mark.parametrize("wb", [11, 12, 13])
def test_the_nt_build_in_packed_cells(genv, wb):
    genv.setenv("FLATGFA_WB", str(wb))
    genv.setenv("FLATGFA_MALL_MB", "0")
    w = 1 << wb
    paths = [chain(300, 3), np.concatenate([np.arange(w - 40, w + 40), shorts(257, w + 100, stride=4, length=3), np.arange(w + 90, w + 900)])]
    check(genv, paths, 2 * w + 11)


# ---- lanes ----

@pytest.mark.parametrize("solo, says", [("0", "shared"), ("1", "solo")])
def test_three_lanes_sweep_packed_cells_shared_and_solo(genv, solo, says):
    """A pipeline of three lanes with the sweep two workgroups to a CU and one (the launch takes half a CU's LDS on top of its
    own): the description names the mode, and the vectors are the oracle's either way -- so equal."""
    from pollen_amd.device import DepthPipeline, DeviceGraph
    genv.setenv("FLATGFA_SORTED_CELLS", "packed")
    genv.setenv("FLATGFA_SORTED_SOLO", solo)
    paths = window_of(300, 0) + [chain(300, 3) + W, long_and_shorts(258) + 2 * W]
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
    m = CELLS.search(desc)
    assert m and m.group(1) == "packed" and m.group(3) == says and " sorted_image_plans=3 " in desc, desc
    for _ in range(2):
        bufs = [buffers(n_segs, uniq=k != 4) for k in range(6)]
        with Profile() as prof:
            for b in bufs:
                pipe.seg_depth(*b)
            pipe.status()
        for k, b in enumerate(bufs):
            assert_right(b, want, k)
    assert prof.pass1() == 0 and prof.pass2() == 6, prof.names
    pipe.close()


def test_a_plan_on_its_own_shares_its_cus_and_the_hook_can_make_it_solo(genv):
    for solo, says in ((None, "shared"), ("1", "solo")):
        if solo:
            genv.setenv("FLATGFA_SORTED_SOLO", solo)
        pools, want = graph_of([chain(300, 3), long_and_shorts(257) + W], 2 * W + 40)
        genv.setenv("FLATGFA_SORTED_CELLS", "packed")
        _, plan, n = plan_of(pools)
        desc = first_call(plan, n, want, "packed")
        assert CELLS.search(desc).group(3) == says, desc
        sweep_calls(plan, n, want)
        plan.close()
