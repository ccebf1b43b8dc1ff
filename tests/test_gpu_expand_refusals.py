"""What chop and inject refuse, by code and by the whole text of flatgfa_last_error: the two features share the driver that
writes these messages (expand_kernels.hpp), and the other suites pin them by code or by a word only.  On a graph of three
segments (2, 5 and 1 bases) under one path of four steps; the totals past 2^32 come from the limit shapes of
tests/chop_shapes.py and tests/inject_shapes.py, which reach them through lengths and line counts, not through memory.  Every
case is a refusal the count is built to make: a flag raised by a guarded kernel, or a check on the host.  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import chop_shapes as cs
import inject_shapes as sh
import pollen_amd as pa
from pollen_amd import _lib
from pollen_amd import device as pdev
from pollen_amd.flatgfa import POOLS
from test_gpu_chop_geometry import count_only as chop_count_only
from test_gpu_chop_geometry import host_handle
from test_gpu_inject_geometry import count_only as inject_count_only

pytestmark = pytest.mark.gpu

LENS = [2, 5, 1]
STEPS = [0 << 1, 1 << 1, 2 << 1, (1 << 1) | 1]  # 13 bases
S, N = len(LENS), len(STEPS)
C = 3
LINE = (0, 1, 6)  # cuts segment 0 at 1 and segment 1 at 4
LINKS = [(0 << 1, 1 << 1), (1 << 1, 2 << 1)]

SPAN = "%s: a path has a step span outside the steps pool"
STEP = "%s: a step refers to a segment id that is out of range"
LINK = "%s: a link refers to a segment id that is out of range"
PATH_ID = "inject: a line names a path id that is out of range"
TOTALS = "%s would have %d segments, %d steps and %d links: more than 32-bit ids hold"


def device_graph(steps=STEPS, end=N):
    return pdev.DeviceGraph(np.array(steps, np.uint32), np.array([0], np.uint32), np.array([end], np.uint32), S, np.array(LENS, np.uint32))


def lines_on_device(lines):
    import torch
    ln = np.array(lines, np.int64).reshape(-1, 3)
    return tuple(torch.from_numpy(ln[:, k].astype(t)).to("cuda:0") for k, t in ((0, np.int32), (1, np.int64), (2, np.int64)))


def refused(call, code, text):
    with pytest.raises(pa.FlatGFAError) as e:
        call()
    assert (e.value.code, _lib.last_error()) == (code, text)


def device_refuses(dg, text, lines=(LINE,), chop=True):
    if chop:
        refused(lambda: pdev.chop(dg, C), -2, text % "chop")
    refused(lambda: pdev.inject(dg, *lines_on_device(lines)), -2, text % "inject" if "%s" in text else text)


def test_a_span_that_ends_past_the_steps_pool():
    device_refuses(device_graph(end=N + 1), SPAN)


def test_a_step_that_names_segment_n_segs():
    device_refuses(device_graph(STEPS[:2] + [S << 1] + STEPS[3:]), STEP)


def test_a_line_that_names_path_n_paths():
    device_refuses(device_graph(), PATH_ID, lines=(LINE, (1, 0, 3)), chop=False)


def test_a_bad_path_id_is_reported_before_a_bad_step():
    # (every read of k_locate and k_line_spans is guarded with both present: the line of no path reads nothing, and a step
    # that names no segment has no bases, so no line end is ever located inside it)
    device_refuses(device_graph(STEPS[:2] + [S << 1] + STEPS[3:]), PATH_ID, lines=(LINE, (1, 0, 3)), chop=False)


def handle(bad_link, bad_step):
    """A FlatGFA of the graph with LINKS, the last of them to segment n_segs when bad_link; with bad_step, step 2 is written
    into the parsed pool afterwards, as host_handle does with the link (the GFA text cannot say either)."""
    links = LINKS[:1] + [(1 << 1, S << 1)] if bad_link else LINKS
    g = host_handle(cs.make_pools(LENS, STEPS, [(0, N)], links))
    if bad_step:
        data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        assert _lib.lib().flatgfa_pool(g._h, POOLS.index("steps"), ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
        assert (n.value, es.value) == (N, 4)
        np.frombuffer((ctypes.c_uint32 * N).from_address(data.value), np.uint32)[2] = S << 1
    return g


@pytest.mark.parametrize("bad_step", [False, True], ids=["link", "step_and_link"])
def test_a_link_to_segment_n_segs_and_a_bad_step_before_it(bad_step):
    g = handle(True, bad_step)
    try:
        text = STEP if bad_step else LINK
        refused(lambda: g.chop(C, True), -2, text % "chop")
        refused(lambda: g.inject([LINE + (b"n0",)], True), -2, text % "inject")
    finally:
        g.close()


def test_totals_past_the_limit_name_every_count():
    rc = chop_count_only(cs.LIMIT_N2[False].arrays(), 1)[0]
    assert (rc, _lib.last_error()) == (-6, TOTALS % ("chop: the chopped graph", 2**31 - 1, 2**32, 0))
    rc, _s, _n, _p, job = inject_count_only(sh.limit(4097))  # 2^20 steps, and 4097 lines that each walk them all
    assert (rc, job, _lib.last_error()) == (-6, None, TOTALS % ("inject: the graph", 16, 4098 << 20, 0))


def test_a_fill_without_steps_after_a_count_that_found_some():
    import torch
    L = _lib.lib()
    dg = device_graph()
    g = dg.c_struct()
    st = ctypes.c_void_p(torch.cuda.current_stream(dg.device).cuda_stream)
    sf = torch.empty(S + 1, dtype=torch.int32, device=dg.device)
    pb, pe = (torch.empty(2, dtype=torch.int32, device=dg.device) for _ in range(2))
    ids, lo, hi = lines_on_device([LINE])
    for what in ("chop", "inject"):
        job = ctypes.c_void_p()
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        if what == "chop":
            rc = L.flatgfa_dev_chop_count(ctypes.byref(g), C, sf.data_ptr(), st, ctypes.byref(job), ctypes.byref(a), ctypes.byref(b))
            fill, free, want = L.flatgfa_dev_chop_fill, L.flatgfa_dev_chop_free, (4, 6)  # 1 + 2 + 1 pieces; 1 + 2 + 1 + 2 steps
        else:
            rc = L.flatgfa_dev_inject_count(ctypes.byref(g), ids.data_ptr(), lo.data_ptr(), hi.data_ptr(), 1, sf.data_ptr(), st,
                                            ctypes.byref(job), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
            fill, free, want = L.flatgfa_dev_inject_fill, L.flatgfa_dev_inject_free, (5, 9)  # 2 + 2 + 1; 2 + 2 + 1 + 2, and 2 new
        try:
            assert rc == 0 and (a.value, b.value) == want, (what, _lib.last_error())
            seg_len = torch.empty(a.value, dtype=torch.int32, device=dg.device)
            rc = fill(job, None, pb.data_ptr(), pe.data_ptr(), seg_len.data_ptr(), st)
            assert (rc, _lib.last_error()) == (-1, what + ": NULL output")
        finally:
            free(job)
