"""What tests/device_check/sorted_image_check.hip cannot reach of the sorted record image, end to end with
the helpers of test_gpu_sorted_groups.py.

The sweep's builds that read past the caches: k_accum_sorted<UNIQ, WB, NT=true> is what a plan runs whose image and results
exceed the cache budget -- every large graph -- and under FLATGFA_MALL_MB=0, which these cases set.  At each window width the
layout of test_runs_across_window_edges_at_every_width and one window of 257 records (a full group and a checked group of one
chunk), through `check`: with unique depth and depth only, bit for bit against the C oracle, in buffers pre-filled with -1.
The description does not say which build ran; that it is the NT one is what the mutant of profiles/NOTES.md shows (a change
confined to sorted_load4<true> fails these cases and no others).

FLATGFA_KEEP_RECORDS=0: a plan that rewrites its records every call gets no image -- `pass2=walk(rewritten)` -- and every call
runs a pass 1.
"""
import numpy as np
import pytest

from test_gpu_sorted_groups import W, check, genv, records_per_window, shorts, window_of  # noqa: F401 (genv is a fixture)
from test_gpu_sorted_records import PASS2, IMAGE, Profile, assert_right, buffers, env, graph_of, plan_of  # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def ntenv(genv):
    genv.setenv("FLATGFA_MALL_MB", "0")
    return genv


@pytest.mark.parametrize("wb", [11, 12, 13])
def test_nt_runs_across_window_edges_at_every_width(ntenv, wb):
    ntenv.setenv("FLATGFA_WB", str(wb))
    w = 1 << wb
    paths = [np.concatenate([np.arange(w - 100, w + 100), np.arange(2 * w - 50, 2 * w + 30), np.arange(w - 10, w + 10), np.arange(w - 3, w), np.arange(w - 700, w),
                             shorts(300, w - 950), shorts(140, w + 2), np.arange(w - 1, w + 1)]),
             np.concatenate([np.arange(w - 60, w + 60), np.arange(w - 1, w + 1), np.arange(2 * w - 40, 2 * w + 30), shorts(90, w - 200), np.arange(w - 1, w)])]
    got = records_per_window(paths, wb)
    assert got[0] > 256 and got[1] > 128 and 0 < got[2] < 64, got
    desc, want = check(paths, 2 * w + 30)
    assert f"x{w} " in desc, desc
    assert want[0][w - 1] > want[1][w - 1] and want[0][2 * w + 29] == 2


@pytest.mark.parametrize("wb", [11, 12, 13])
def test_nt_a_window_of_257_records_at_every_width(ntenv, wb):
    """Window 0 has 257 records (ids below 2048: the same at every width): a full group, then a checked group of one chunk with
    one record and 63 of padding."""
    ntenv.setenv("FLATGFA_WB", str(wb))
    w = 1 << wb
    paths = window_of(257, 0)
    assert max(int(p.max()) for p in paths) < 2048
    assert records_per_window(paths, wb)[0] == 257
    desc, want = check(paths, w + 17)
    assert f"x{w} " in desc, desc
    assert (want[0][:900] > want[1][:900]).any()


def test_a_plan_that_rewrites_its_records_keeps_the_walk(genv):
    genv.setenv("FLATGFA_KEEP_RECORDS", "0")
    paths = window_of(257, 0) + window_of(70, 2 * W, other_path=False, pos=sum(len(p) for p in window_of(257, 0)))
    pools, want = graph_of(paths, 3 * W + 17)
    _, plan, n_segs = plan_of(pools)
    b = buffers(n_segs)
    plan.seg_depth(*b)
    plan.status()
    assert_right(b, want, "first call")
    desc = plan.describe()
    m = PASS2.search(desc)
    assert IMAGE.search(desc) and m and m.group(1) == "walk(rewritten)" and m.group(3) == "rewritten", desc
    bufs = [buffers(n_segs), buffers(n_segs, uniq=False), buffers(n_segs), buffers(n_segs)]
    with Profile() as prof:
        for x in bufs:
            plan.seg_depth(*x)
        plan.status()
    for k, x in enumerate(bufs):
        assert_right(x, want, f"call {k}")
    assert (prof.count("k_scan_runs"), prof.pass1(), prof.pass2()) == (4, 4, 4), prof.names
    plan.close()
