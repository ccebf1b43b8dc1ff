"""chop on the GPU at the kernels' tile edges and 32-bit limits (the shapes of tests/chop_shapes.py): the device entry
(device.chop) on every shape, FlatGFA.chop with and without links on those with sequence data, `fgfa chop` on the
scan shapes past 2^20 elements, two streams at once, a chopped graph handed to a depth plan, and S' = 2^31 - 1 /
N' = 2^32 - 1 written and checked on the device in closed form.  Run with -m gpu."""
import ctypes
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import chop_model as cm
import chop_shapes as cs
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from pollen_amd import device as pdev
from pollen_amd.flatgfa import POOLS

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
CATALOG = cs.catalog(full=True)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def device_graph(p: fo.Pools):
    lens = (p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"].astype(np.int64)).astype(np.uint32)
    return pdev.DeviceGraph(p.steps, p.paths["steps_start"], p.paths["steps_end"], len(p.segs), lens)


def check_device_result(p, c, dg, sf, want):
    assert np.array_equal(u32(sf), cm.seg_first(p, c).astype(np.uint32))
    assert np.array_equal(u32(dg.steps), want.steps)
    assert np.array_equal(u32(dg.path_begin), want.paths["steps_start"])
    assert np.array_equal(u32(dg.path_end), want.paths["steps_end"])
    assert np.array_equal(u32(dg.seg_len), (want.segs["seq_end"] - want.segs["seq_start"]).astype(np.uint32))


def check_device(s: cs.Shape):
    if s.err is not None:
        with pytest.raises(pa.FlatGFAError) as e:
            pdev.chop(device_graph(s.pools), s.c)
        assert e.value.code == s.err, s.name
        return None
    dg, sf = pdev.chop(device_graph(s.pools), s.c)
    check_device_result(s.pools, s.c, dg, sf, cm.chop_fast(s.pools, s.c))
    return dg, sf


def params(tiling):
    return [pytest.param(f, id=name) for name, f, t, _ in CATALOG if t == tiling]


# (split by layout: the tiling kernels and the per-path ones can be run apart)
@pytest.mark.parametrize("factory", params(True))
def test_device_tiling_shapes(factory):
    check_device(factory())


@pytest.mark.parametrize("factory", params(False))
def test_device_per_path_shapes(factory):
    check_device(factory())


@pytest.mark.parametrize("c", cs.F_CS)
def test_device_u64_lengths(c):
    s = cs.f_shape(c)
    first, new_len, steps = cs.f_expect(cs.f_lens(c), c)
    dg, sf = pdev.chop(device_graph(s.pools), c)
    assert u32(sf).tolist() == first
    assert u32(dg.seg_len).tolist() == new_len
    assert u32(dg.steps).tolist() == steps
    assert u32(dg.path_begin).tolist() == [0] and u32(dg.path_end).tolist() == [len(steps)]


def bad_link(p: fo.Pools):
    S = len(p.segs)
    bad = np.nonzero(((p.links["from_"] >> 1) >= S) | ((p.links["to"] >> 1) >= S))[0]
    return int(bad[0]) if len(bad) else None


def host_handle(p: fo.Pools):
    """A FlatGFA with exactly these pools.  The loader refuses a link past the segments, so a graph with one is parsed with
    that link made valid, and the link is then written back into the parsed (heap) pool."""
    bad = bad_link(p)
    if bad is None:
        fd, path = tempfile.mkstemp(suffix=".flatgfa")
        with os.fdopen(fd, "wb") as f:
            f.write(fo.dump_flatgfa(p))
        try:
            return pa.load(path)
        finally:
            os.unlink(path)
    ok = fo.Pools(**{n: getattr(p, n).copy() for n in fo.POOL_ORDER})
    ok.links[bad] = (0, 0, 0, 0)
    g = pa.parse_bytes(cm.text(ok))
    data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, POOLS.index("links"), ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
    assert n.value == len(p.links) and es.value == 16
    lk = np.frombuffer((ctypes.c_uint32 * (n.value * 4)).from_address(data.value), np.uint32).reshape(-1, 4)
    lk[bad, 0], lk[bad, 1] = p.links[bad]["from_"], p.links[bad]["to"]
    assert bad_link(cm.pools_of(g)) == bad
    return g


# (all but the spans outside the pool, which the loader refuses: the device entry has them)
@pytest.mark.parametrize("factory", [pytest.param(f, id=name) for name, f, _, host in CATALOG if host])
def test_host_shapes(factory):
    s = factory()
    g = host_handle(s.pools)
    try:
        p = cm.pools_of(g)
        for links in (False, True):
            err = s.err_links if links else s.err
            if err is not None:
                with pytest.raises(pa.FlatGFAError) as e:
                    g.chop(s.c, links)
                assert e.value.code == err, (s.name, links)
                continue
            q = g.chop(s.c, links)
            assert cm.same_pools(cm.pools_of(q), cm.chop_fast(p, s.c, links)), (s.name, links)
            q.close()
    finally:
        g.close()


@pytest.mark.parametrize("n", [n for n in cs.SCAN_FULL if n >= cs.CARRY])
@pytest.mark.parametrize("kind", ["segs", "steps", "paths"])
def test_cli_past_two_to_the_20(kind, n):
    s = {"segs": cs.a_segs, "steps": cs.a_steps, "paths": cs.a_paths}[kind](n)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "in.flatgfa")
        with open(path, "wb") as f:
            f.write(fo.dump_flatgfa(s.pools))
        r = subprocess.run([FGFA, "-i", path, "chop", "-c", str(s.c)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == cm.text(cm.chop_fast(s.pools, s.c))


def test_two_streams():
    import torch
    shapes = [cs.a_segs(cs.CARRY + 4097, seed=1), cs.a_paths(cs.CARRY + 1, seed=1)]
    graphs = [device_graph(s.pools) for s in shapes]
    streams = [torch.cuda.Stream() for _ in shapes]
    out, errs = [None, None], []

    def run(k):
        try:
            with torch.cuda.stream(streams[k]):
                out[k] = [pdev.chop(graphs[k], shapes[k].c, stream=streams[k]) for _ in range(3)]
        except Exception as e:  # (reported below, on the main thread)
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for s, res in zip(shapes, out):
        want = cm.chop_fast(s.pools, s.c)
        for dg, sf in res:
            check_device_result(s.pools, s.c, dg, sf, want)


def test_depth_past_two_to_the_20_segments():
    import torch
    s = cs.a_segs(cs.CARRY + 4097, seed=2)
    p = s.pools
    d_old, u_old = fo.seg_depth_with_uniq(p)
    dg, sf = check_device(s)
    S2 = dg.n_segs
    assert S2 > cs.CARRY
    depth = torch.zeros(S2, dtype=torch.int32, device=dg.device)
    uniq = torch.zeros(S2, dtype=torch.int32, device=dg.device)
    plan = pdev.DepthPlan(dg, first=(depth, uniq))
    try:
        assert plan.first_status == 0
        old = np.repeat(np.arange(len(p.segs)), np.diff(u32(sf).astype(np.int64)))
        assert np.array_equal(u32(depth).astype(np.uint64), d_old[old].astype(np.uint64))
        assert np.array_equal(u32(uniq).astype(np.uint64), u_old[old].astype(np.uint64))
    finally:
        plan.close()


# ---- G: the 32-bit limits ----
def count_only(arrays, c):
    """flatgfa_dev_chop_count alone (nothing is filled): (code, S', N', seg_first)."""
    import torch
    steps, b, e, S, lens = arrays
    dg = pdev.DeviceGraph(steps, b, e, S, lens)
    sf = torch.full((S + 1,), -1, dtype=torch.int32, device=dg.device)
    g = dg.c_struct()
    job = ctypes.c_void_p()
    n1, n2 = ctypes.c_uint64(), ctypes.c_uint64()
    L = _lib.lib()
    rc = L.flatgfa_dev_chop_count(ctypes.byref(g), c, ctypes.c_void_p(sf.data_ptr()),
                                  ctypes.c_void_p(torch.cuda.current_stream(dg.device).cuda_stream), ctypes.byref(job),
                                  ctypes.byref(n1), ctypes.byref(n2))
    L.flatgfa_dev_chop_free(job)
    torch.cuda.synchronize()
    return rc, n1.value, n2.value, u32(sf).tolist()


@pytest.mark.parametrize("trailing", [False, True], ids=["tiling", "per_path"])
def test_limit_counts(trailing):
    ok, over = cs.LIMIT_OK[trailing], cs.LIMIT_N2[trailing]
    assert count_only(ok.arrays(), 1) == (0, 2**31 - 1, 2**32 - 1, ok.seg_first())
    assert count_only(over.arrays(), 1)[0] == cs.ERR_TOO_LARGE  # N' = 2^32
    assert count_only(cs.limit_s2_refused(), 1)[0] == cs.ERR_TOO_LARGE  # S' = 2^31


@pytest.mark.parametrize("trailing", [False, True], ids=["tiling", "per_path"])
def test_limit_fill_two_to_the_32_minus_1_steps(trailing):
    # 16 GB of steps and 8 GB of seg_len; with trailing, k_expand_paths writes all 2^32 - 1 steps from one 256-step chunk
    import torch
    lim = cs.LIMIT_OK[trailing]
    dg, sf = pdev.chop(pdev.DeviceGraph(*lim.arrays()), 1)
    try:
        assert (dg.n_segs, dg.n_steps) == (lim.S2, lim.N2)
        assert u32(sf).tolist() == lim.seg_first()
        assert u32(dg.path_begin).tolist() == [0] and u32(dg.path_end).tolist() == [lim.N2]
        chunk = 1 << 28
        for t, n, f in ((dg.steps, lim.N2, lim.steps_at), (dg.seg_len, lim.S2, lim.seg_len_at)):
            for s0 in range(0, n, chunk):
                j = torch.arange(s0, min(s0 + chunk, n), dtype=torch.int64, device=dg.device)
                got = t[s0:s0 + len(j)].to(torch.int64) & 0xFFFFFFFF
                bad = torch.nonzero(got != f(j))
                assert bad.numel() == 0, (s0 + int(bad[0]), n)
                del j, got, bad
    finally:
        del dg, sf
        torch.cuda.empty_cache()
