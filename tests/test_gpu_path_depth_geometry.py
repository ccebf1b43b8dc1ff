"""Path depth on the GPU with long segments (the shapes of tests/path_depth_shapes.py): every 64-bit sum the kernels form
carries into its upper word somewhere -- the window prefix table, a run record, a lane's share, a wave's total, the
per-window partials, the pieces of a split path, the gather kernel's thread, wave and block sums.  Every shape goes through
the device entry (DeviceGraph with seg_len, DepthPlan.path_depth_all, twice on one plan) on the fused route and on each
fallback, and the route is asserted from the profiled kernel names, not assumed; then 8-record buckets (the call is run again
inside status()), path_sums on its own in request order, a pipeline of three lanes, and the host API, `fgfa depth` and virtual
shards on a .flatgfa image whose segments alias one sequence pool.  length and weighted are compared as exact integers with
tests/path_depth_model.py, the mean bitwise.  Run with -m gpu."""
import functools
import os
import subprocess

import numpy as np
import pytest

import path_depth_model as pm
import path_depth_shapes as ps
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
HOOKS = ("FLATGFA_DEPTH_PATH", "FLATGFA_BUCKET_CAP", "FLATGFA_PIECE_STEPS", "FLATGFA_SHORT_MAX", "FLATGFA_SHORT_ANY", "FLATGFA_ACC_PARTS",
         "FLATGFA_RANGE_SEGS", "FLATGFA_DENSE", "FLATGFA_BIG_GROUPS", "FLATGFA_TAGGED", "FLATGFA_NO_CLAIM", "FLATGFA_SCAN_WGS",
         "FLATGFA_PATH_GROUPS", "FLATGFA_PACKED", "FLATGFA_ACC_SLOTS", "FLATGFA_WB", "FLATGFA_ACC_OWN", "FLATGFA_TAG_LIMIT")
FUSED = [f.__name__ for f in ps.FUSED] + ["mixed", "host_long"]
FALLBACKS = {
    "atomic": {"FLATGFA_DEPTH_PATH": "atomic"},  # the global-atomic kernels
    "packed": {"FLATGFA_DEPTH_PATH": "bucketed", "FLATGFA_PACKED": "1", "FLATGFA_SHORT_MAX": "0", "FLATGFA_ACC_PARTS": "1",
               "FLATGFA_DENSE": "0"},  # buckets laid out to the count (pass 1 by runs: the partitioning pass 1 keeps the even layout): tagged calls only
    "ranges": {"FLATGFA_DEPTH_PATH": "bucketed", "FLATGFA_RANGE_SEGS": "8192"},  # one walk of the steps per range of 8192 segments: every shape has at least two
    "parts3": {"FLATGFA_DEPTH_PATH": "bucketed", "FLATGFA_ACC_PARTS": "3"},  # a window's final depth is in no one workgroup
}


def torch():
    import torch as t
    return t


@functools.lru_cache(maxsize=None)
def n_cus() -> int:
    return torch().cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def shape(name: str) -> ps.Shape:
    return dict(ps.catalog(n_cus()))[name]()


@functools.lru_cache(maxsize=None)
def want(name: str):
    """(length, weighted) as lists of Python ints, the mean's bytes, the depth."""
    s = shape(name)
    a = pm.exact(*s.graph()) if len(s.steps) <= ps.EXACT_MAX_STEPS else pm.twin(*s.graph())
    return [int(x) for x in a.length], [int(x) for x in a.weighted], a.mean.tobytes(), a.depth.astype(np.uint32)


def set_env(monkeypatch, env) -> None:
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)


def fused_env(s: ps.Shape) -> dict:
    """The fused route on a graph of a few windows: the bucketed path whatever the plan's timing says, one pass-2 workgroup
    per window, and (unless the shape is about the plan's own classes) every path an item of k_scan."""
    env = {"FLATGFA_DEPTH_PATH": "bucketed", "FLATGFA_ACC_PARTS": "1"}
    if s.short_max0:
        env["FLATGFA_SHORT_MAX"] = "0"
    env.update(dict(s.env))
    return env


def device_graph(s: ps.Shape) -> pdev.DeviceGraph:
    return pdev.DeviceGraph(s.steps, s.begin, s.end, s.n_segs, s.seg_len)


def outputs(g: pdev.DeviceGraph):
    """Output buffers full of ones: a sum that is not cleared, or a path nobody writes, shows."""
    t = torch()
    return (t.full((g.n_segs,), -1, dtype=t.int32, device="cuda"), t.full((g.n_paths,), -1, dtype=t.int64, device="cuda"),
            t.full((g.n_paths,), -1, dtype=t.int64, device="cuda"))


def check(name: str, d, ln, ws, what) -> None:
    w_len, w_w, w_mean, w_d = want(name)
    got_l = ln.cpu().numpy().view(np.uint64).tolist()
    got_w = ws.cpu().numpy().view(np.uint64).tolist()
    bad = [(p, got_l[p], w_len[p], got_w[p], w_w[p]) for p in range(len(w_len)) if (got_l[p], got_w[p]) != (w_len[p], w_w[p])]
    assert not bad, (name, what, len(bad), "(path, length got / want, weighted got / want)", bad[:4])
    assert (d.cpu().numpy().view(np.uint32) == w_d).all(), (name, what, "depth")
    assert pm.means(got_l, got_w).tobytes() == w_mean, (name, what, "mean")


def run_all(name: str, plan: pdev.DepthPlan, what, calls: int = 2):
    """path_depth_all `calls` times on one plan (its scratch and the outputs' zeroing are reused), each checked whole; returns the
    names of the kernels the first call ran, one per launch, in launch order."""
    g = plan.graph
    names = None
    for k in range(calls):
        d, ln, ws = outputs(g)
        if k == 0:
            pdev.profile_enable(True)
            pdev.profile_read()
        try:
            plan.path_depth_all(d, ln, ws)
            plan.status()
        finally:
            if k == 0:
                pdev.profile_enable(False)
                names = [n for n, _ in pdev.profile_read()]
        if k == 0:
            print(name, what, names, plan.describe())  # (shown when the case fails)
        check(name, d, ln, ws, (what, "call %d" % k))
    return names


@pytest.mark.parametrize("name", FUSED)
def test_fused_route(name, monkeypatch):
    s = shape(name)
    set_env(monkeypatch, fused_env(s))
    plan = pdev.DepthPlan(device_graph(s))
    try:
        names = run_all(name, plan, "fused")
        assert "k_path_reduce" in names and "k_accum<depth+paths>" in names, (name, sorted(names), plan.describe())
        if not s.short_max0:  # the plan's own classes: the wave-per-path kernels' paths take the gather kernel
            assert "k_path_sums" in names, (name, sorted(names), plan.describe())
        else:
            assert "k_path_sums" not in names, (name, sorted(names))
    finally:
        plan.close()


def fallback_params():
    """Every fused shape on every fallback; the gather shapes (one window or two: no ranges to be had) on the atomic kernels and
    with three workgroups a window, where path_depth_all requests every path by_path."""
    return [pytest.param(n, c, id="%s-%s" % (n, c)) for n in FUSED for c in FALLBACKS] + \
           [pytest.param(n, c, id="%s-%s" % (n, c)) for n in ("gather_lengths", "gather_levels") for c in ("atomic", "parts3")]


@pytest.mark.parametrize("name,config", fallback_params())
def test_fallback_routes(name, config, monkeypatch):
    s = shape(name)
    set_env(monkeypatch, dict(FALLBACKS[config], **dict(s.env)))
    plan = pdev.DepthPlan(device_graph(s))
    try:
        names = run_all(name, plan, config)
        what = plan.describe()
        if config == "packed" and "buckets=packed" not in what:
            # FLATGFA_PACKED=1 asks, the plan decides (depth_fast.hip: can_pack, and whether the layout its counting call
            # finds fits): a plan that says it kept the even layout is not a fallback, and must say so and run the fused route
            assert "buckets=even" in what and "path=bucketed" in what and "workgroups_per_window=1 " in what, what
            assert "k_path_reduce" in names and "k_accum<depth+paths>" in names, (name, names, what)
            return
        assert "k_path_sums" in names and "k_path_reduce" not in names, (name, config, names, what)
        if config == "atomic":
            assert "path=atomic" in what
        elif config == "packed":
            assert "pass2=tagged" in what, what
        elif config == "ranges":
            assert s.n_segs > 8192 and "ranges=1 " not in plan.describe(), plan.describe()
        elif config == "parts3":
            assert "workgroups_per_window=3" in plan.describe(), plan.describe()
    finally:
        plan.close()


def test_large_windows_take_the_gather_kernel(monkeypatch):
    s = shape("large_windows")
    set_env(monkeypatch, {"FLATGFA_DEPTH_PATH": "bucketed"})
    plan = pdev.DepthPlan(device_graph(s))
    try:
        names = run_all("large_windows", plan, "wb13")
        assert "x8192" in plan.describe(), plan.describe()
        assert "k_path_sums" in names and "k_path_reduce" not in names, (sorted(names), plan.describe())
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["wave_totals", "many_items", "split_paths", "reverse_nonmonotone", "mixed"])
def test_tiny_buckets_run_the_call_again(name, monkeypatch):
    """8-record sub-buckets overflow: status() finds the call incomplete and runs path_depth_all again into the same outputs
    (a plan with a forced capacity cannot grow: through the atomic kernels and k_path_sums over every path).  What the first
    attempt added to the sums must not be counted on top.  That the second attempt took place is read from the launches:
    the sums are cleared (memset_path_sums) and gathered again BEHIND the fused pass 2 of the same call."""
    s = shape(name)
    set_env(monkeypatch, dict(fused_env(s), FLATGFA_BUCKET_CAP="8"))
    plan = pdev.DepthPlan(device_graph(s))
    try:
        names = run_all(name, plan, "tinycap", calls=3)
        assert "k_accum<depth+paths>" in names, (names, plan.describe())
        first = names.index("k_accum<depth+paths>")
        assert "memset_path_sums" in names[first:], (names, plan.describe())
        again = first + names[first:].index("memset_path_sums")
        assert "k_path_sums" in names[again:], (names, plan.describe())
    finally:
        plan.close()


def request_params():
    return [pytest.param(n, r, id="%s-%s" % (n, r)) for n in ("gather_lengths", "gather_levels") for r, _ in dict(ps.catalog())[n]().requests]


@pytest.mark.parametrize("name,request_name", request_params())
@pytest.mark.parametrize("path", ["bucketed", "atomic"])
def test_path_sums_in_request_order(name, request_name, path, monkeypatch):
    """flatgfa_dev_path_sums on its own: results in the order of the request, repeated ids each credited in full."""
    t = torch()
    s = shape(name)
    ids = np.array(dict(s.requests)[request_name], np.uint32)
    split = pm.split_of(len(ids), n_cus())
    if request_name in ("one", "split64"):
        assert split == ps.MAX_SPLIT
    elif request_name.startswith("split1") or request_name == "several":
        assert split == 1
    else:
        assert 1 < split <= ps.MAX_SPLIT
    set_env(monkeypatch, {"FLATGFA_DEPTH_PATH": path})
    w_len, w_w, _, w_d = want(name)
    g = device_graph(s)
    plan = pdev.DepthPlan(g)
    try:
        d = t.full((g.n_segs,), -1, dtype=t.int32, device="cuda")
        plan.seg_depth(d, None)
        plan.status()
        assert (d.cpu().numpy().view(np.uint32) == w_d).all()
        dq = t.from_numpy(ids.view(np.int32)).cuda()
        for call in range(2):
            ln = t.full((len(ids),), -1, dtype=t.int64, device="cuda")
            ws = t.full((len(ids),), -1, dtype=t.int64, device="cuda")
            pdev.profile_enable(True)
            pdev.profile_read()
            try:
                plan.path_sums(dq, d, ln, ws)
                plan.status()
            finally:
                pdev.profile_enable(False)
                names = {n for n, _ in pdev.profile_read()}
            assert "k_path_sums" in names and "k_path_reduce" not in names
            got_l, got_w = ln.cpu().numpy().view(np.uint64).tolist(), ws.cpu().numpy().view(np.uint64).tolist()
            bad = [(k, int(p), got_l[k], w_len[p], got_w[k], w_w[p]) for k, p in enumerate(ids.tolist()) if (got_l[k], got_w[k]) != (w_len[p], w_w[p])]
            assert not bad, (name, request_name, call, len(bad), bad[:4])
    finally:
        plan.close()


def test_pipeline_of_three_lanes(monkeypatch):
    """Seven calls through three lanes (each lane a plan of its own, two or three calls a lane), each into buffers of its own."""
    s = shape("prefix_len")
    set_env(monkeypatch, fused_env(s))
    g = device_graph(s)
    pipe = pdev.DepthPipeline(g, 3)
    try:
        outs = [outputs(g) for _ in range(7)]
        for d, ln, ws in outs:
            pipe.path_depth_all(d, ln, ws)
        pipe.status()
        for k, (d, ln, ws) in enumerate(outs):
            check("prefix_len", d, ln, ws, ("pipeline", k, pipe.describe()))
    finally:
        pipe.close()


# ---- the host ABI: long segments in a .flatgfa image ----
@functools.lru_cache(maxsize=None)
def host_pools() -> fo.Pools:
    """host_long as pools whose segments' sequence spans alias one pool of 4 MiB (flatgfa_load checks that a span lies inside
    its pool, not that spans are disjoint): 9000 segments of up to 2^22 bases cost 4 MiB, not 23 GB."""
    s = shape("host_long")
    p = ps.pools_of(s)
    p.seq_data = np.full(1 << 22, ord("A"), np.uint8)
    assert int(p.segs["seq_end"].max()) <= len(p.seq_data) and (p.segs["seq_start"] == 0).all()
    return p


@pytest.fixture
def host_image(tmp_path, monkeypatch):
    set_env(monkeypatch, {})
    f = str(tmp_path / "long.flatgfa")
    with open(f, "wb") as out:
        out.write(fo.dump_flatgfa(host_pools()))
    return f


def test_host_api_and_cli_with_long_segments(host_image):
    w_len, w_w, w_mean, _ = want("host_long")
    pools = host_pools()
    o_len, o_mean = fo.path_depth(pools)
    assert o_len.tolist() == w_len and o_mean.tobytes() == w_mean and min(w_len[:4]) >= 1 << 32
    g = pa.load(host_image)
    try:
        ln, mean = g.path_depth()
        assert ln.tolist() == w_len and mean.tobytes() == w_mean
        ids = [5, 3, 0, 3, 4, 1]
        ln, mean = g.path_depth(ids)
        assert ln.tolist() == [w_len[p] for p in ids] and mean.tobytes() == np.frombuffer(w_mean, np.float64)[ids].tobytes()
        assert g.path_depth_table() == fo.fgfa_depth(pools, False)
    finally:
        g.close()
    out = subprocess.run([FGFA, "-i", host_image, "depth"], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout == fo.fgfa_depth(pools, False)


@pytest.mark.parametrize("n_shards", [2, 3])
def test_virtual_shards_with_long_segments(host_image, n_shards):
    """Each shard's sums are its own call's; the host adds them up: a path cut between shards has parts below and a total
    above 2^32."""
    w_len, _, w_mean, _ = want("host_long")
    g = pa.load(host_image)
    try:
        with pa.ShardedFlatGFA(g, n_shards, devices=[0] * n_shards) as sh:
            for _ in range(2):
                ln, mean = sh.path_depth()
                assert ln.tolist() == w_len and mean.tobytes() == w_mean
            ln, mean = sh.path_depth([2, 0, 2])
            assert ln.tolist() == [w_len[2], w_len[0], w_len[2]]
            assert mean.tobytes() == np.frombuffer(w_mean, np.float64)[[2, 0, 2]].tobytes()
    finally:
        g.close()
