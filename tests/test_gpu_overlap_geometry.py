"""Path overlap on the GPU at the kernels' grid strides, coarse blocks, LDS windows, query batches and limits (the shapes of
tests/overlap_shapes.py): the device entry (DepthPlan.path_overlaps) on every shape in both bitset modes and from step
arrays that do not start on a 16-byte line, the host API and `fgfa overlap --paths` past the batch and stride thresholds,
out-of-range ids, sequences of calls on one plan, two plans on two streams, and the 2^28-segment limit and its refusals.
Every answer is checked whole, against the shape's closed form or tests/overlap_model.py.  Run with -m gpu."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import overlap_model as om
import overlap_shapes as osh
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev
from test_overlap_model import emit, pools

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
HOOK = "FLATGFA_OVERLAP_DENSE_MAX"


def torch():
    import torch as t
    return t


@functools.lru_cache(maxsize=None)
def n_cus() -> int:
    return torch().cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def shape(name: str) -> osh.Shape:
    return dict(osh.catalog(n_cus()))[name]()


@functools.lru_cache(maxsize=None)
def want(name: str) -> np.ndarray:
    s = shape(name)
    return s.want if s.want is not None else om.touch_sparse(s.steps, s.begin, s.end, s.n_segs, s.queries)


def device_graph(s: osh.Shape, steps=None, offset: int = 0, seg_len=None) -> pdev.DeviceGraph:
    """The shape on the device; offset k > 0: its steps are a view at element k of a larger buffer (a base that is not 16-byte
    aligned), the elements around it the bait handle."""
    steps = s.steps if steps is None else steps
    if offset == 0:
        return pdev.DeviceGraph(steps, s.begin, s.end, s.n_segs, seg_len)
    t = torch()
    N = len(steps)
    buf = t.full((N + 8,), int(steps[0]), dtype=t.int32, device="cuda")
    buf[offset:offset + N] = t.from_numpy(steps.view(np.int32)).cuda()
    pb = t.from_numpy(s.begin.view(np.int32)).cuda()
    pe = t.from_numpy(s.end.view(np.int32)).cuda()
    g = pdev.DeviceGraph.from_tensors(buf[offset:offset + N], pb, pe, s.n_segs, h_path_begin=s.begin, h_path_end=s.end)
    assert g.steps.data_ptr() % 16 == 4 * offset % 16
    return g


def overlaps(plan: pdev.DepthPlan, queries, stream=None) -> np.ndarray:
    """One call on torch's current stream (or `stream`), waited for, status checked: uint8[n_q, P]."""
    t = torch()
    q = np.ascontiguousarray(queries, np.uint32)
    P = plan.graph.n_paths
    with t.cuda.stream(stream or t.cuda.current_stream()):
        dq = t.from_numpy(q.view(np.int32)).cuda()
        out = t.full((len(q) * P,), 0xAB, dtype=t.uint8, device="cuda")
        plan.path_overlaps(dq, out)
        plan.status()
        return out.cpu().numpy().reshape(len(q), P)


def set_mode(monkeypatch, mode: str) -> None:
    if mode == "queries":
        monkeypatch.setenv(HOOK, "0")  # exact bitsets of the queries only: candidates are walked step by step
    else:
        monkeypatch.delenv(HOOK, raising=False)


@pytest.fixture
def atomic(monkeypatch):
    # (the plan's own depth path allocates nothing per segment: a plan of 2^28 segments and more is cheap)
    monkeypatch.setenv("FLATGFA_DEPTH_PATH", "atomic")
    monkeypatch.delenv(HOOK, raising=False)


def device_params():
    out = []
    for name, _ in osh.catalog():
        big = name.startswith("limit")
        for offset in ((0, 3) if big else (0, 1, 2, 3)):
            out.append(pytest.param(name, "default", offset, id="%s-default-%d" % (name, offset)))
        if name not in ("grid_batches", "batch_edges", "limit"):  # (those are queries-only by size already)
            out.append(pytest.param(name, "queries", 0, id="%s-queries-0" % name))
            if not big:
                out.append(pytest.param(name, "queries", 3, id="%s-queries-3" % name))
    return out


@pytest.mark.parametrize("name,mode,offset", device_params())
def test_device_shapes(name, mode, offset, atomic, monkeypatch):
    s = shape(name)
    set_mode(monkeypatch, mode)
    assert osh.all_paths(s.n_segs, s.P, 0 if mode == "queries" else osh.DENSE) == (mode == "default" and name not in
                                                                                     ("grid_batches", "batch_edges", "limit"))
    plan = pdev.DepthPlan(device_graph(s, offset=offset))
    try:
        got = overlaps(plan, s.queries)
        bad = np.argwhere(got != want(name))
        assert len(bad) == 0, (name, mode, offset, len(bad), bad[:8].tolist())
    finally:
        plan.close()


def test_grid_shapes_past_the_strides_on_this_device():
    from test_overlap_model import reaches
    r = reaches(shape("grid_batches"), n_cus())
    assert all(r[k] for k in ("coarse_stride", "bits_stride", "pair_stride", "ballot_round_2", "windows_3", "batches_3")), r
    r = reaches(shape("grid_dense"), n_cus())
    assert r["dense"] and r["bits_stride"] and r["coarse_stride"] and r["pair_stride"], r


@pytest.mark.parametrize("S", osh.REFUSED)
def test_refused_past_two_to_the_28_segments(S, atomic):
    s = osh.refused(S)
    plan = pdev.DepthPlan(device_graph(s))  # (a plan of this many segments is made: only the overlap call refuses)
    t = torch()
    try:
        out = t.full((4,), 0xAB, dtype=t.uint8, device="cuda")
        with pytest.raises(pa.FlatGFAError) as e:
            plan.path_overlaps(t.tensor([0, 1], dtype=t.int32, device="cuda"), out)
        assert e.value.code == osh.ERR_TOO_LARGE, S
        plan.status()
        assert out.cpu().tolist() == [0xAB] * 4  # nothing written
    finally:
        plan.close()


def test_zero_segments(atomic):
    s = osh.Shape("empty", np.zeros(0, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint32), 0, np.array([2, 0], np.uint32))
    plan = pdev.DepthPlan(device_graph(s))
    try:
        assert not overlaps(plan, s.queries).any()
    finally:
        plan.close()


# ---- the host API and the CLI, past the batch and stride thresholds ----
def named_pools(s: osh.Shape) -> fo.Pools:
    """The shape as a whole graph: segments 1..S of one base, paths p0, p1, ..."""
    p = pools(s.steps, s.begin, s.end, s.n_segs)
    p.segs["name"] = np.arange(1, s.n_segs + 1)
    p.segs["seq_start"] = np.arange(s.n_segs)
    p.segs["seq_end"] = np.arange(1, s.n_segs + 1)
    p.seq_data = np.full(s.n_segs, ord("A"), np.uint8)
    names = [b"p%d" % i for i in range(s.P)]
    ln = np.array([len(n) for n in names])
    p.paths["name_end"] = np.cumsum(ln)
    p.paths["name_start"] = p.paths["name_end"] - ln
    p.name_data = np.frombuffer(b"".join(names), np.uint8).copy()
    return p


def test_host_api_and_cli_past_the_thresholds():
    s = shape("grid_batches")
    p = named_pools(s)
    assert osh.batches(s.n_segs, s.P, len(s.queries)) != [(0, len(s.queries))]
    w = want("grid_batches")
    table = emit(p, s.queries, w)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "g.flatgfa")
        with open(path, "wb") as f:
            f.write(fo.dump_flatgfa(p))
        names = os.path.join(d, "q.paths")
        with open(names, "wb") as f:
            f.write(b"".join(b"p%d\n" % q for q in s.queries))
        g = pa.load(path)
        try:
            assert np.array_equal(g.path_overlaps(s.queries), w)
            assert g.overlap_table([b"p%d" % q for q in s.queries]) == table
        finally:
            g.close()
        r = subprocess.run([FGFA, "-i", path, "overlap", "--paths", names], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table


# ---- out-of-range ids ----
@pytest.mark.parametrize("mode", ["default", "queries"])
@pytest.mark.parametrize("where", ["query", "candidate"])
def test_bad_segment_id_then_a_valid_call(where, mode, atomic, monkeypatch):
    set_mode(monkeypatch, mode)
    s = shape("step_layout")
    bad_path = 1 if where == "query" else 40  # (a query path with planted handles, and a candidate with steps)
    assert s.end[bad_path] > s.begin[bad_path]
    steps = s.steps.copy()
    steps[s.begin[bad_path]] = 2 * s.n_segs  # segment id == n_segs
    ok = s.steps.copy()
    ok[s.begin[bad_path]] = 2 * s.n_segs - 1  # (a handle nobody else has: what a kernel that skips the bad step sees)
    assert not np.isin(ok[s.begin[bad_path]], np.delete(s.steps, s.begin[bad_path]))
    others = np.array([q for q in s.queries if q != bad_path], np.uint32)
    first = s.queries if where == "query" else others
    plan = pdev.DepthPlan(device_graph(s, steps=steps))
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            overlaps(plan, first)
        assert e.value.code == osh.ERR_BOUNDS
        got = overlaps(plan, others[::-1])  # the next valid call on the same plan
        assert np.array_equal(got, om.touch_sparse(ok, s.begin, s.end, s.n_segs, others[::-1]))
    finally:
        plan.close()


def test_bad_query_id(atomic):
    s = shape("orientation")
    plan = pdev.DepthPlan(device_graph(s))
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            overlaps(plan, [0, s.P, 1])
        assert e.value.code == osh.ERR_BOUNDS
        assert np.array_equal(overlaps(plan, s.queries), want("orientation"))
    finally:
        plan.close()


# ---- sequences of calls on one plan ----
def model(s, steps, q):
    return om.touch_sparse(steps, s.begin, s.end, s.n_segs, q)


def test_modes_in_turn(atomic, monkeypatch):
    s = shape("edges")
    plan = pdev.DepthPlan(device_graph(s))
    rng = np.random.default_rng(1)
    try:
        for mode in ("default", "queries", "default", "queries"):
            set_mode(monkeypatch, mode)
            q = rng.permutation(s.queries)[: int(rng.integers(5, len(s.queries)))]
            assert np.array_equal(overlaps(plan, q), model(s, s.steps, q)), mode
    finally:
        plan.close()


def test_queries_only_with_every_path_then_all_paths(atomic, monkeypatch):
    # the cache is big enough for every path but laid out by query (here in reverse path order): all-paths mode rebuilds it
    for name in ("edges", "step_layout"):
        s = shape(name)
        plan = pdev.DepthPlan(device_graph(s))
        try:
            rev = np.arange(s.P, dtype=np.uint32)[::-1].copy()
            set_mode(monkeypatch, "queries")
            assert np.array_equal(overlaps(plan, rev), model(s, s.steps, rev))
            set_mode(monkeypatch, "default")
            assert np.array_equal(overlaps(plan, s.queries), want(name)), name
        finally:
            plan.close()


@pytest.mark.parametrize("mode", ["default", "queries"])
def test_query_sets_that_shrink_and_grow(mode, atomic, monkeypatch):
    set_mode(monkeypatch, mode)
    s = shape("batch_edges" if mode == "default" else "edges")
    plan = pdev.DepthPlan(device_graph(s))
    try:
        n = len(s.queries)
        for k in (3, 1, n, 2, n // 2 + 1, n):
            q = s.queries[n - k:] if k % 2 else s.queries[:k]
            assert np.array_equal(overlaps(plan, q), model(s, s.steps, q)), k
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ["default", "queries"])
def test_steps_changed(mode, atomic, monkeypatch):
    set_mode(monkeypatch, mode)
    t = torch()
    s = shape("edges")
    g = device_graph(s)
    plan = pdev.DepthPlan(g)
    try:
        assert np.array_equal(overlaps(plan, s.queries), want("edges"))
        new = s.steps.copy()
        rng = np.random.default_rng(5)
        inside = np.concatenate([np.arange(b, e) for b, e in zip(s.begin, s.end)])
        pick = rng.choice(inside, 40, replace=False)
        new[pick] = new[rng.choice(inside, 40)]  # new handles shared between paths, old ones gone
        new[pick[:10]] = rng.integers(2 * (1 << 21), 2 * s.n_segs, 10)  # and some in blocks of the later ballot rounds
        g.steps.copy_(t.from_numpy(new.view(np.int32)).cuda())
        plan.steps_changed()
        w = model(s, new, s.queries)
        assert not np.array_equal(w, want("edges"))
        assert np.array_equal(overlaps(plan, s.queries), w)
    finally:
        plan.close()


def test_interleaved_with_depth(monkeypatch):
    monkeypatch.delenv("FLATGFA_DEPTH_PATH", raising=False)
    monkeypatch.delenv(HOOK, raising=False)
    t = torch()
    s = shape("orientation")
    p = pools(s.steps, s.begin, s.end, s.n_segs)
    p.segs["seq_end"] = 1
    wd, wu = fo.seg_depth_with_uniq(p)
    plan = pdev.DepthPlan(device_graph(s, seg_len=np.ones(s.n_segs, np.uint32)))
    try:
        d = t.zeros(s.n_segs, dtype=t.int32, device="cuda")
        u = t.zeros_like(d)
        ln = t.zeros(s.P, dtype=t.int64, device="cuda")
        wt = t.zeros_like(ln)
        for i in range(3):
            plan.seg_depth(d, u)
            q = s.queries[i::2]
            assert np.array_equal(overlaps(plan, q), want("orientation")[i::2])
            assert np.array_equal(d.cpu().numpy().view(np.uint32), wd) and np.array_equal(u.cpu().numpy().view(np.uint32), wu)
            d.zero_()
            plan.path_depth_all(d, ln, wt)
            assert np.array_equal(overlaps(plan, s.queries), want("orientation"))
            plan.status()
            assert np.array_equal(d.cpu().numpy().view(np.uint32), wd)
            assert np.array_equal(ln.cpu().numpy(), (s.end - s.begin).astype(np.int64))
    finally:
        plan.close()


def test_two_plans_two_streams(atomic):
    t = torch()
    s = shape("grid_dense")
    g = device_graph(s)
    plans = [pdev.DepthPlan(g), pdev.DepthPlan(g)]
    streams = [t.cuda.Stream(), t.cuda.Stream()]
    qs = [s.queries, s.queries[::-1].copy()]
    out, errs = [None, None], []

    def run(k):
        try:
            out[k] = [overlaps(plans[k], qs[k], streams[k]) for _ in range(3)]
        except Exception as e:  # (reported below, on the main thread)
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        for k in range(2):
            for got in out[k]:
                assert np.array_equal(got, want("grid_dense")[::-1] if k else want("grid_dense"))
    finally:
        for pl in plans:
            pl.close()
