"""What a depth plan's creation launches: the timed trials of plan_build_fast (depth_device.hip), seen through the per-launch
profiling records (`pollen_amd.device.profile_enable` / `profile_read` bracket every launch, plan creation's included).

A plan is made by running the query itself: once to size the record buckets, then -- where the graph leaves a choice open --
a few more times per variant, the faster one kept.  Which variant wins is timing; HOW OFTEN each one is launched is not, and
that is what these tests pin: the counts below were taken from the library as it was before plan_build_fast was cut into
stages, and each follows from the rules in the comment beside it.  Every case's answer is compared with the C oracle bit for
bit, so a trial that left a plan in a wrong shape shows up here as well.

The graphs are hand-made: 24 paths of 4000 steps on 3000 segments (96 000 steps), every path a sequence of runs of
consecutive segment ids whose lengths cycle through a pattern.  With runs of ten (400 a path) single waves walk the paths
(`k_scan_medium`); with runs of one and two (2667 a path: more than a wave's hash set takes) they are k_scan's items, and
pass 1 is `k_scan` or `k_scan_dense`.
"""
import collections
import dataclasses
import os
import re

import numpy as np
import pytest

import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

S, P, L = 3000, 24, 4000

# The rules (plan_build_fast), for a plan made without `first`, whose scratch outputs always have a uniq half:
#   sizing       one bucketed query, and one more each time the record buckets had to grow (twice on these graphs: three queries)
#   pass 1       dense_maybe (more than a record for two steps) in every range: 3 repetitions x {k_scan, k_scan_dense}
#   shortcut     untagged and FLATGFA_BIG_GROUPS unset: 3 repetitions x {item by item, one-item shortcut} = 6 bucketed queries
#   atomic       no variable that shapes the plan is set and at most 8 M steps: 4 bucketed queries, then 4 atomic ones
# and FLATGFA_DEPTH_PATH=atomic makes no bucketed plan at all: the atomic kernels run once if the caller wants a first answer.
UNIQ_PATH_UNSHAPED = 4        # the four atomic repetitions of the bucketed-vs-atomic trial
UNIQ_PATH_BUCKETED = 0        # FLATGFA_DEPTH_PATH=bucketed is a shaped plan: no comparison
UNIQ_PATH_ATOMIC_FIRST = 1    # no bucketed plan, one first answer (atomic_first)
UNIQ_PATH_ATOMIC = 0          # ... and none without `first`
PASS1_TRIAL_REPS = 3          # k_scan and k_scan_dense each run at least their three trial repetitions.  The totals of the shaped
                              # (bucketed) plan below: sizing runs the plan's default, k_scan_dense, three times -> k_scan 3, k_scan_dense 6
                              # whichever wins; where by runs wins on a plan whose workgroups take many items each, the bitset-owner
                              # trial adds 6 of k_scan (not here: 24 items on 24 workgroups)
SHORTCUT_TRIAL_CALLS = 6      # pass 2 runs six more times than with FLATGFA_BIG_GROUPS=1, which takes the trial's place

# what the sizing and timing runs decide (tests/test_gpu_depth.py strips the same fields as timing-dependent)
TIMING_FIELDS = r" (pass1|bucket_cap|scratch_mb)=\S+|\(one-item shortcut\)| bitset_owners=tracked"


def _steps(pattern):
    """P paths of L forward steps: runs of consecutive ids, their lengths cycling through `pattern`, each starting at a
    pseudo-random segment (oracle.synth's mix64: the same on every machine)."""
    lens = np.resize(np.asarray(pattern, dtype=np.int64), L)  # (more runs than needed: cut to L steps below)
    first = np.cumsum(lens) - lens
    out = np.zeros((P, L), dtype=np.uint32)
    for p in range(P):
        with np.errstate(over="ignore"):
            key = np.uint64(1 + p) * synth.GOLDEN + np.arange(L, dtype=np.uint64)
        start = (synth.mix64(key) % np.uint64(S - max(pattern))).astype(np.int64)
        ids = np.repeat(start, lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
        out[p] = (ids[:L] << 1).astype(np.uint32)
    return out.reshape(-1)


@pytest.fixture(scope="module")
def cases():
    """name -> (pools, oracle depth, oracle uniq); computed once, never written to."""
    base = synth.pools(5, S, P, L)
    made = {}
    for name, pattern in (("runs10", (10,)), ("runs1and2", (1, 2))):
        pools = dataclasses.replace(base, steps=_steps(pattern))
        want_d, want_u = fo.seg_depth_with_uniq(pools)
        made[name] = (pools, want_d, want_u)
    return made


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("FLATGFA_") and k != "FLATGFA_LIB":
            monkeypatch.delenv(k)
    return monkeypatch


def _graph(pools, device="cuda:0"):
    from pollen_amd.device import DeviceGraph
    return DeviceGraph(pools.steps, pools.paths["steps_start"], pools.paths["steps_end"], S, device=device)


def _profiled(fn):
    """The names of the kernels `fn` launches, counted."""
    from pollen_amd import device as dev
    dev.profile_read()
    dev.profile_enable(True)
    try:
        result = fn()
    finally:
        dev.profile_enable(False)
    return result, collections.Counter(name for name, _ in dev.profile_read())


def _create(pools, first=None):
    from pollen_amd.device import DepthPlan
    graph = _graph(pools)
    return _profiled(lambda: DepthPlan(graph, first=first))


def _buffers(device="cuda:0"):
    import torch
    return (torch.full((S,), -1, dtype=torch.int32, device=device), torch.full((S,), -1, dtype=torch.int32, device=device))


def _same(t, want):
    return (t.cpu().numpy().view(np.uint32) == want).all()


def _check_next_answer(plan, case, device="cuda:0"):
    _, want_d, want_u = case
    d, u = _buffers(device)
    plan.seg_depth(d, u)
    plan.status()  # (raises unless OK)
    assert _same(d, want_d) and _same(u, want_u), plan.describe()


def test_unshaped_plan_times_bucketed_against_atomic(cases, clean_env):
    plan, names = _create(cases["runs10"][0])
    print("unshaped:", dict(names), plan.describe())
    assert names["k_depth_uniq_path"] == UNIQ_PATH_UNSHAPED, names
    _check_next_answer(plan, cases["runs10"])
    plan.close()


def test_shaped_plan_skips_the_comparison(cases, clean_env):
    clean_env.setenv("FLATGFA_DEPTH_PATH", "bucketed")
    plan, names = _create(cases["runs10"][0])
    print("bucketed:", dict(names), plan.describe())
    assert names["k_depth_uniq_path"] == UNIQ_PATH_BUCKETED, names
    assert "path=bucketed" in plan.describe() and " pass2=tagged" in plan.describe(), plan.describe()
    _check_next_answer(plan, cases["runs10"])
    plan.close()


def test_atomic_plan_runs_once_for_a_first_answer(cases, clean_env):
    clean_env.setenv("FLATGFA_DEPTH_PATH", "atomic")
    pools, want_d, want_u = cases["runs10"]
    d, u = _buffers()
    plan, names = _create(pools, first=(d, u))
    print("atomic, first:", dict(names))
    assert names["k_depth_uniq_path"] == UNIQ_PATH_ATOMIC_FIRST, names
    assert plan.first_status == 0 and _same(d, want_d) and _same(u, want_u)
    plan.status()
    plan.close()
    plan, names = _create(pools)
    print("atomic:", dict(names))
    assert names["k_depth_uniq_path"] == UNIQ_PATH_ATOMIC, names
    assert plan.describe().startswith("path=atomic")
    _check_next_answer(plan, cases["runs10"])
    plan.close()


def test_dense_maybe_plan_times_both_forms_of_pass_1(cases, clean_env):
    clean_env.setenv("FLATGFA_DEPTH_PATH", "bucketed")
    pools, want_d, want_u = cases["runs1and2"]
    d, u = _buffers()
    plan, names = _create(pools, first=(d, u))
    print("dense_maybe:", dict(names), plan.describe())
    assert names["k_scan"] >= PASS1_TRIAL_REPS and names["k_scan_dense"] >= PASS1_TRIAL_REPS, names
    assert plan.first_status == 0 and _same(d, want_d) and _same(u, want_u), plan.describe()  # (every trial wrote the same counts)
    plan.status()
    _check_next_answer(plan, cases["runs1and2"])
    plan.close()


def test_untagged_plan_times_the_one_item_shortcut(cases, clean_env):
    clean_env.setenv("FLATGFA_TAGGED", "0")
    pass2 = {}
    for forced in (None, "1"):
        if forced:
            clean_env.setenv("FLATGFA_BIG_GROUPS", forced)
        plan, names = _create(cases["runs10"][0])
        print("untagged, FLATGFA_BIG_GROUPS =", forced, dict(names), plan.describe())
        assert " pass2=directory" in plan.describe() and names["k_depth_uniq_path"] == 0, (plan.describe(), names)
        pass2[forced] = sum(n for name, n in names.items() if name.startswith("k_accum"))
        _check_next_answer(plan, cases["runs10"])
        plan.close()
    assert pass2[None] - pass2["1"] == SHORTCUT_TRIAL_CALLS, pass2


def test_steps_changed_makes_the_plan_the_same_way(cases, clean_env):
    plan, names = _create(cases["runs10"][0])
    before = re.sub(TIMING_FIELDS, "", plan.describe())
    _, again = _profiled(plan.steps_changed)
    after = re.sub(TIMING_FIELDS, "", plan.describe())
    print("steps_changed:", dict(again), after)
    assert again == names, (names, again)
    assert after == before, (before, after)
    _check_next_answer(plan, cases["runs10"])
    plan.close()


def test_steps_changed_and_describe_leave_the_callers_device_current(cases, clean_env):
    import torch
    from pollen_amd import _lib
    from pollen_amd.device import DepthPlan
    if pa.device_count() < 2:
        pytest.skip("needs two devices")
    plan = DepthPlan(_graph(cases["runs10"][0], device="cuda:1"))
    torch.cuda.set_device(0)
    # (through the C ABI: DepthPlan's methods switch to the plan's device and back themselves)
    assert _lib.lib().flatgfa_dev_plan_steps_changed(plan._p, None) == 0
    assert torch.cuda.current_device() == 0
    assert plan.describe().startswith("path=") and torch.cuda.current_device() == 0
    _check_next_answer(plan, cases["runs10"], device="cuda:1")
    assert torch.cuda.current_device() == 0
    plan.close()
