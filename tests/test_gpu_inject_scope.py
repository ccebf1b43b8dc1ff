"""The device scope of flatgfa_inject (DevScope in pollen_amd/csrc/capi.cpp), seen from outside on one tiny graph, as
tests/test_gpu_dev_scope.py does for the other routes: a call that is refused part-way -- by the count on the device, after the
uploads -- gives back what it held (the next call on the handle answers as the model does), a handle answers the same before
and after it becomes resident, and two hundred calls in turn with other routes leave the stream pool sound.  Every refusal here
is an error return.  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import chop_model as cm
import inject_model as im
import pollen_amd as pa
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_BOUNDS, ERR_TOO_LARGE = -1, -2, -6

GFA = (b"S\t1\tACGT\nS\t2\tAC\nS\t3\tGGA\nS\t4\tT\nS\t5\tCCCCA\nS\t6\tTG\nS\t7\tA\nS\t8\tGATTACA\n"
       b"P\tx\t1+,2+,3+,4+,5+\t*\nP\ty\t1+,3+,4-,6+,8+\t*\nP\tz\t7+,8-,2+\t*\n"
       b"L\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nL\t4\t+\t5\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t7\t+\t8\t-\t0M\n")
LINES = [(b"x", 2, 9, b"a"), (b"y", 5, 12, b"b"), (b"z", 3, 6, b"c"), (b"x", 0, 15, b"d")]


def inject_ids(g, ids, lo, hi, names, links=1):
    n = len(ids)
    a, b, c = np.array(ids, np.uint32), np.array(lo, np.uint64), np.array(hi, np.uint64)
    cn = (ctypes.c_char_p * max(n, 1))(*names)
    cl = (ctypes.c_size_t * max(n, 1))(*[len(x) for x in names])
    h = ctypes.c_void_p()
    rc = _lib.lib().flatgfa_inject(g._h, a.ctypes.data, b.ctypes.data, c.ctypes.data, cn, cl, n, links, ctypes.byref(h))
    return rc, (pa.FlatGFA(h.value) if h.value else None)


def test_refused_part_way_and_asked_again():
    g = pa.parse_bytes(GFA)
    want = im.inject(cm.pools_of(g), LINES, links=True)
    for resident in (False, True):
        if resident:
            g.to_device()
        # refused by the count, after the graph and the lines were uploaded: a path id out of range
        rc, h = inject_ids(g, [0, 3], [1, 1], [5, 5], [b"a", b"b"])
        assert rc == ERR_BOUNDS and h is None and "path id" in _lib.last_error()
        # refused before the device: a name twice
        rc, h = inject_ids(g, [0, 1], [1, 1], [5, 5], [b"a", b"a"])
        assert rc == ERR_ARG and h is None
        rc, h = inject_ids(g, [0, 1, 2, 0], [ln[1] for ln in LINES], [ln[2] for ln in LINES], [ln[3] for ln in LINES])
        assert rc == 0 and cm.same_pools(cm.pools_of(h), want)
        assert cm.same_pools(cm.pools_of(g.inject(im.bed_text(LINES), links=True)), want)
    # the result is a handle of its own: it outlives the input and takes every route
    g.close()
    assert cm.same_pools(cm.pools_of(h.chop(2, True)), cm.chop(want, 2, True))
    again = h.inject([(b"a", 1, 3, b"aa")])
    assert cm.same_pools(cm.pools_of(again), im.inject(want, [(b"a", 1, 3, b"aa")]))


def test_a_refused_total_gives_everything_back():
    # 4 097 lines that each cover a path of 2^20 steps: refused by the count's totals, then a small call on the same handle
    n = 1 << 20
    g = pa.parse_bytes(b"S\t1\tA\nP\tp\t" + b",".join([b"1+"] * n) + b"\t*\n")
    rc, h = inject_ids(g, [0] * 4097, [0] * 4097, [n] * 4097, [b"n%d" % i for i in range(4097)], links=0)
    assert rc == ERR_TOO_LARGE and h is None and "steps" in _lib.last_error()
    rc, h = inject_ids(g, [0], [5], [9], [b"q"], links=0)
    assert rc == 0 and h.path_count == 2 and len(cm.pools_of(h).steps) == n + 4


def test_two_hundred_calls_in_turn_with_other_routes():
    g = pa.parse_bytes(GFA)
    p = cm.pools_of(g)
    want = im.inject(p, LINES, links=True)
    chopped = cm.chop(p, 2, True)
    bed = im.bed_text(LINES)
    for i in range(200):
        if i % 3 == 0:
            assert cm.same_pools(cm.pools_of(g.chop(2, True)), chopped)
        elif i % 3 == 1:
            assert cm.same_pools(cm.pools_of(g.inject(bed, links=True)), want)
        else:
            rc, h = inject_ids(g, [7], [1], [5], [b"a"])
            assert rc == ERR_BOUNDS and h is None
