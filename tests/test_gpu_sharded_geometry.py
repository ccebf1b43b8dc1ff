"""The sharded engine (flatgfa_sharded_*, pollen_amd/csrc/sharded.hip) at the edges of its packing, its cut rule and its
grids (the shapes of tests/sharded_shapes.py): more cut paths than one packed word holds, a count that fills its field, more
segments than one trip of the fix-up kernels, 64 shards, paths out of pool order, sequences of calls and two threads on one
handle, every documented refusal, and the RCCL route.  The layout is compared with tests/sharded_model.py's field by
field, every answer whole with the shape's closed form or the model.  All shards share device 0 (the exchange is the
device-side add) but for one case that needs two devices.  Run with -m gpu."""
import contextlib
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import pollen_amd as pa
import sharded_model as sm
import sharded_shapes as ss
from conftest import ROOT
from oracle import flatgfa_oracle as fo

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def loaded(s: ss.Shape):
    """The shape as a graph of the library's, through a .flatgfa image (the only way in for spans out of pool order)."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "shape.flatgfa")
        with open(path, "wb") as f:
            f.write(fo.dump_flatgfa(ss.pools(s.graph)))
        with pa.load(path) as g:
            yield g


class Want:
    """What the model says of a shape: the layout, the reduced vectors (the closed form where the shape has one, which
    must be the model's too) and the path depths."""

    def __init__(self, s: ss.Shape):
        self.lay = sm.layout(s.graph, s.n_shards, s.flags)
        self.depth, self.uniq, _ = sm.exchange(s.graph, self.lay)
        if s.depth is not None:
            assert (self.depth == s.depth).all() and (self.uniq == s.uniq).all()
            self.depth, self.uniq = s.depth, s.uniq
        if s.K is not None:
            assert (self.lay.K, self.lay.W) == (s.K, s.W)
        self.len, self.mean = sm.path_depth(s.graph, self.lay, self.depth)


def check_layout(sh, lay: sm.Layout, devices, rccl=False):
    got = sh.layout()
    assert len(got) == lay.n_shards
    for r, (x, m) in enumerate(zip(got, lay.shards)):
        assert x == {"device": devices[r], "step_begin": m.step_begin, "step_end": m.step_end, "first_path": m.first_path,
                     "pieces": len(m.pieces), "split_paths": lay.K, "rccl": rccl}, r
    assert sh.collective_bytes(True) == lay.collective_bytes(True)
    assert sh.collective_bytes(False) == lay.collective_bytes(False)
    assert sh.ranks_seen() == lay.n_shards


def check_answers(sh, w: Want):
    d, u = sh.seg_depth_with_uniq()
    assert (d == w.depth).all(), "depth"
    assert (u == w.uniq).all(), "uniq"
    assert (sh.seg_depth() == w.depth).all(), "seg_depth"
    ln, mean = sh.path_depth()
    assert (ln == w.len).all(), "path lengths"
    assert mean.tobytes() == w.mean.tobytes(), "mean depth (bitwise, NaN included)"
    sh.enqueue(True)
    sh.sync()
    for i in range(w.lay.n_shards):
        d, u = sh.fetch(i)
        assert (d == w.depth).all() and (u == w.uniq).all(), f"shard {i} holds another vector"


def check_shape(s: ss.Shape):
    w = Want(s)
    devices = [0] * s.n_shards
    with loaded(s) as g, pa.ShardedFlatGFA(g, s.n_shards, devices=devices, flags=s.flags) as sh:
        check_layout(sh, w.lay, devices)
        check_answers(sh, w)
    return w


# ---- the packing ----
@pytest.mark.parametrize("P,n_shards,K,W", ss.RINGS_MULTIWORD)
def test_rings_with_more_cut_paths_than_one_word_holds(P, n_shards, K, W):
    """K = 10, 15 and 49 cut paths in W = 2, 3 and 13 words per segment: the word index, the last field of a word and the
    first of the next.  The last case is the documented maximum of 64 shards."""
    w = check_shape(ss.ring_multiword(P, n_shards, K, W))
    assert (w.lay.K, w.lay.W) == (K, W)


@pytest.mark.parametrize("n_shards", ss.RING_SINGLE)
def test_one_path_in_n_shards_pieces(n_shards):
    """Every one of the n_shards pieces touches every segment: the count is n_shards, the top bit of its field at 2, 4, ...
    64, and the fix-up takes n_shards - 1 off."""
    w = check_shape(ss.ring_single(n_shards))
    assert [len(x.pieces) for x in w.lay.shards] == [1] * n_shards and (w.uniq == 1).all()


@pytest.mark.parametrize("P,n_shards,K,W", ss.RINGS_MULTIWORD[:2] + [(1, 16, 1, 1), (3, 16, 3, 1), (5, 4, 3, 1)])
def test_spokes_whose_pieces_touch_different_segments(P, n_shards, K, W):
    """Counts from 0 to the number of pieces over the segments of one cut path, different in every field of a word."""
    check_shape(ss.spokes(P, n_shards, K, W))


def test_whole_paths_flag_on_a_shape_that_would_be_cut():
    s = ss.ring_multiword(12, 13, 10, 2)._replace(flags=pa.SHARD_WHOLE_PATHS, K=0, W=0)
    w = check_shape(s)
    assert sorted(len(x.pieces) for x in w.lay.shards) == [0] + [1] * 12


# ---- the grids ----
def test_more_segments_than_one_trip_of_the_fix_up_grids():
    """2048 * 256 + 300 segments, three paths cut in two on four shards: k_pack_touch and k_fix_uniq stride a second time,
    and the segments they reach there are touched by both pieces of two paths."""
    s = ss.wide()
    assert s.graph.S > ss.GRID_SEGS
    w = check_shape(s)
    assert (w.uniq == 3).all() and (w.depth == 6).all() and w.lay.K == 3


# ---- paths out of pool order ----
@pytest.mark.parametrize("n_shards", [2, 5])
@pytest.mark.parametrize("kind", ss.OUT_OF_ORDER)
def test_paths_out_of_pool_order_are_never_cut(kind, n_shards):
    s = ss.out_of_order(kind, n_shards)
    w = check_shape(s)
    assert w.lay.ordered == s.ordered and (s.ordered or w.lay.K == 0)
    pools = ss.pools(s.graph)  # (the oracle walks the spans as they are)
    want_d, want_u = fo.seg_depth_with_uniq(pools)
    assert (w.depth == want_d).all() and (w.uniq == want_u).all()


# ---- sequences of calls on one handle ----
@pytest.mark.parametrize("shape", ["ring", "spokes"])
def test_call_sequences_on_one_handle(shape):
    s = ss.ring_multiword(12, 13, 10, 2) if shape == "ring" else ss.spokes(19, 20, 15, 3)
    w = Want(s)
    P = s.graph.P
    with loaded(s) as g, pa.ShardedFlatGFA(g, s.n_shards, devices=[0] * s.n_shards) as sh:
        # depth only, with unique depth, depth only, ...: k_pack_touch ORs into the packed words, which every call must find zeroed
        for with_uniq in (False, True, False, True, True, False):
            if with_uniq:
                d, u = sh.seg_depth_with_uniq()
                assert (d == w.depth).all() and (u == w.uniq).all()
            else:
                assert (sh.seg_depth() == w.depth).all()
        # unique depth cannot be fetched after a call that did not compute it
        sh.enqueue(False)
        sh.sync()
        with pytest.raises(pa.FlatGFAError) as ei:
            sh.fetch(0, with_uniq=True)
        assert ei.value.code == ss.ERR_ARG
        for i in (0, s.n_shards - 1):
            assert (sh.fetch(i, with_uniq=False) == w.depth).all()
        sh.enqueue(True)
        sh.sync()
        for i in range(s.n_shards):
            d, u = sh.fetch(i)
            assert (d == w.depth).all() and (u == w.uniq).all()
        # path depth (a depth-only call inside) for subsets, repeated ids, ids in descending order
        for ids in ([3], [P - 1, 0], list(range(P - 1, -1, -1)), [5, 5, 5, 2, 5], [], [0, P - 1] * 7):
            ln, mean = sh.path_depth(ids)
            at = np.array(ids, np.int64)
            assert (ln == w.len[at]).all() and mean.tobytes() == w.mean[at].tobytes(), ids
        with pytest.raises(pa.FlatGFAError) as ei:
            sh.fetch(0, with_uniq=True)  # (path depth was the last call)
        assert ei.value.code == ss.ERR_ARG
        for bad in ([P], [0, 1, P], [0xFFFFFFFF]):
            with pytest.raises(pa.FlatGFAError) as ei:
                sh.path_depth(bad)
            assert ei.value.code == ss.ERR_BOUNDS
        check_answers(sh, w)


def test_two_threads_on_one_handle():
    """seg_depth_with_uniq and path_depth (which runs a depth-only call) from two threads at once, twenty times each: a call is
    one critical section from its enqueue to its copy out, so every result is whole."""
    s = ss.spokes(12, 13, 10, 2)
    w = Want(s)
    with loaded(s) as g, pa.ShardedFlatGFA(g, s.n_shards, devices=[0] * s.n_shards) as sh:
        got = {"uniq": [], "path": [], "err": []}

        def uniq():
            try:
                for _ in range(20):
                    got["uniq"].append(sh.seg_depth_with_uniq())
            except Exception as e:  # (reported below: an exception in a thread would otherwise go unseen)
                got["err"].append(e)

        def path():
            try:
                for _ in range(20):
                    got["path"].append(sh.path_depth())
            except Exception as e:
                got["err"].append(e)

        ts = [threading.Thread(target=uniq), threading.Thread(target=path)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(300)
            assert not t.is_alive()
        assert not got["err"], got["err"]
        assert len(got["uniq"]) == 20 and len(got["path"]) == 20
        for d, u in got["uniq"]:
            assert (d == w.depth).all() and (u == w.uniq).all()
        for ln, mean in got["path"]:
            assert (ln == w.len).all() and mean.tobytes() == w.mean.tobytes()
        check_answers(sh, w)


# ---- refusals ----
def test_refusals_leave_the_graph_and_the_handle_usable():
    s = ss.ring_multiword(12, 13, 10, 2)
    w = Want(s)
    n = s.n_shards
    with loaded(s) as g:
        for bad_n in (0, 65):
            with pytest.raises(pa.FlatGFAError, match="bad argument"):
                pa.ShardedFlatGFA(g, bad_n, devices=[0] * bad_n)
        ndev = pa.device_count()
        for devices in ([0] * (n - 1) + [ndev], [ndev] + [0] * (n - 1), [0] * (n - 1) + [-1]):
            with pytest.raises(pa.FlatGFAError, match="device index out of range"):
                pa.ShardedFlatGFA(g, n, devices=devices)
        with pa.ShardedFlatGFA(g, n, devices=[0] * n) as sh:
            for shard in (n, -1, 64):
                with pytest.raises(pa.FlatGFAError) as ei:
                    sh.fetch(shard)
                assert ei.value.code == ss.ERR_ARG
            with pytest.raises(pa.FlatGFAError) as ei:
                sh.path_depth([s.graph.P])
            assert ei.value.code == ss.ERR_BOUNDS
            check_layout(sh, w.lay, [0] * n)
            check_answers(sh, w)


# ---- RCCL ----
def test_rccl_route_with_one_shard(monkeypatch):
    """FLATGFA_SHARD_FORCE_RCCL=1: a communicator of size one, ncclAllReduce from send to recv, and shard_exchange's own
    branch.  One shard cuts nothing (K == 0), so the fix-up has nothing to do there; the answers are exact."""
    monkeypatch.setenv("FLATGFA_SHARD_FORCE_RCCL", "1")
    for s in (ss.ring(12, 960, 24, 1, 0, 0), ss.spokes(5, 1, 0, 0), ss.out_of_order("reversed", 1)):
        w = Want(s)
        assert w.lay.K == 0
        with loaded(s) as g, pa.ShardedFlatGFA(g, 1, devices=[0]) as sh:
            check_layout(sh, w.lay, [0], rccl=True)
            assert sh.layout()[0]["split_paths"] == 0
            check_answers(sh, w)
            check_answers(sh, w)


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import pollen_amd as pa, sharded_shapes as ss, test_gpu_sharded_geometry as t
s = ss.ring(3, 960, 24, 2, 1, 1)  # (the even cut lies in the middle of the second path)
w = t.Want(s)
flags = int(sys.argv[2])
with t.loaded(s) as g, pa.ShardedFlatGFA(g, 2, devices=[0, 1], flags=flags) as sh:
    t.check_layout(sh, w.lay, [0, 1], rccl=not flags)
    t.check_answers(sh, w)
s = ss.ring_single(2)
w = t.Want(s)
with t.loaded(s) as g, pa.ShardedFlatGFA(g, 2, devices=[0, 1], flags=flags) as sh:
    t.check_layout(sh, w.lay, [0, 1], rccl=not flags)
    t.check_answers(sh, w)
print("two devices ok", flags)
"""


def test_two_devices():
    """Shards on devices 0 and 1: the peer-copy bounce of the device-side adds (FLATGFA_SHARD_NO_RCCL) first, then RCCL across
    devices.  Each runs in a child process under a time limit, so that a collective that does not return ends the case."""
    if pa.device_count() < 2:
        pytest.skip(f"needs two HIP devices; this machine shows {pa.device_count()}")
    for flags in (pa.SHARD_NO_RCCL, 0):
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(flags)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "two devices ok" in r.stdout, (flags, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
