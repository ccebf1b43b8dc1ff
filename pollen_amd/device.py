"""Device-level depth queries on caller-owned HBM buffers (Part 3 of include/flatgfa.h).

torch is used for what it is good at here -- device memory, streams, torch.distributed -- and
nothing else: the tensors below are plain int32 buffers whose ``data_ptr()`` goes straight
into the C ABI; every kernel that runs is a hand-written HIP kernel in libflatgfa.so.

Handles are u32 in the reference (flatgfa.rs:186-209); they are carried in torch.int32
tensors because u32 and i32 have the same bits and wrapping add, and int32 is what RCCL and
every torch op accept.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .flatgfa import FlatGFAError, _check


def _torch():
    import torch
    return torch


def _as_i32(a: np.ndarray):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


class DeviceGraph:
    """The structure-of-arrays graph image resident in one GPU's HBM."""

    def __init__(self, steps: np.ndarray, path_begin: np.ndarray, path_end: np.ndarray, n_segs: int,
                 seg_len: Optional[np.ndarray] = None, device: str = "cuda:0"):
        torch = _torch()
        if not torch.cuda.is_available():
            raise FlatGFAError("no HIP device is visible; pollen_amd has no CPU fallback", -3)
        self.device = torch.device(device)
        self.n_steps = int(len(steps))
        self.n_paths = int(len(path_begin))
        self.n_segs = int(n_segs)
        self.h_path_begin = np.ascontiguousarray(path_begin, dtype=np.uint32)
        self.h_path_end = np.ascontiguousarray(path_end, dtype=np.uint32)
        with torch.cuda.device(self.device):
            self.steps = _as_i32(steps).to(self.device)
            self.path_begin = _as_i32(self.h_path_begin).to(self.device)
            self.path_end = _as_i32(self.h_path_end).to(self.device)
            self.seg_len = None if seg_len is None else _as_i32(seg_len).to(self.device)
            torch.cuda.synchronize(self.device)

    @classmethod
    def from_tensors(cls, steps, path_begin, path_end, n_segs: int, seg_len=None,
                     h_path_begin: Optional[np.ndarray] = None, h_path_end: Optional[np.ndarray] = None) -> "DeviceGraph":
        """A DeviceGraph over int32 CUDA tensors that are already on the device (kept, not copied).  The host copies of the
        spans (what a DepthPlan hands the C ABI) are copied back from the device when not given."""
        torch = _torch()
        for t in (steps, path_begin, path_end) + (() if seg_len is None else (seg_len,)):
            assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.device == steps.device
        assert path_begin.numel() == path_end.numel() and (seg_len is None or seg_len.numel() == n_segs)
        g = cls.__new__(cls)
        g.device = steps.device
        g.n_steps, g.n_paths, g.n_segs = int(steps.numel()), int(path_begin.numel()), int(n_segs)
        g.steps, g.path_begin, g.path_end, g.seg_len = steps, path_begin, path_end, seg_len
        g.h_path_begin = (np.ascontiguousarray(h_path_begin, dtype=np.uint32) if h_path_begin is not None
                          else path_begin.cpu().numpy().view(np.uint32).copy())
        g.h_path_end = (np.ascontiguousarray(h_path_end, dtype=np.uint32) if h_path_end is not None
                        else path_end.cpu().numpy().view(np.uint32).copy())
        return g

    def c_struct(self) -> _lib.flatgfa_dev_graph_t:
        return _lib.flatgfa_dev_graph_t(
            self.steps.data_ptr() if self.n_steps else None, self.n_steps,
            self.path_begin.data_ptr() if self.n_paths else None,
            self.path_end.data_ptr() if self.n_paths else None, self.n_paths, self.n_segs,
            self.seg_len.data_ptr() if self.seg_len is not None and self.n_segs else None)


class DepthPlan:
    """A prepared depth query (flatgfa_dev_plan_t): launch plan + scratch HBM for one DeviceGraph.

    The plan is laid out for the step values it was made with: a caller that changes ``graph.steps`` (a mutable
    tensor) under a live plan calls :meth:`steps_changed` before the next query -- a path the plan found strictly
    monotone is counted without the per-path "seen" set, and nothing re-checks that per call (``FLATGFA_CHECK_NO_CLAIM=1``
    in the environment does, as a debugging aid: ``status()`` then raises with code -8).

    ``first=(depth_out, uniq_out)`` (int32 CUDA tensors of n_segs elements; uniq_out may be None): the query that sizes
    the plan's scratch writes the caller's buffers -- creating the plan is the first query (flatgfa_dev_plan_create_first);
    the tensors are complete when the constructor returns, and ``first_status`` is 0 or -2 (an id out of range)."""

    def __init__(self, graph: DeviceGraph, first=None):
        torch = _torch()
        self.graph = graph
        self.first_status = 0
        with torch.cuda.device(graph.device):
            g = graph.c_struct()
            hb = graph.h_path_begin.ctypes.data if graph.n_paths else None
            he = graph.h_path_end.ctypes.data if graph.n_paths else None
            if first is None:
                self._p = ctypes.c_void_p(_lib.lib().flatgfa_dev_plan_create(ctypes.byref(g), hb, he))
            else:
                d, u = first
                S = graph.n_segs
                for t in (d, u):
                    if t is not None:
                        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == S
                torch.cuda.current_stream(graph.device).synchronize()  # (the plan's creation runs on the null stream: whatever filled the buffers is done first)
                st = ctypes.c_int(0)
                self._p = ctypes.c_void_p(_lib.lib().flatgfa_dev_plan_create_first(
                    ctypes.byref(g), hb, he, d.data_ptr() if S else None, u.data_ptr() if (u is not None and S) else None, ctypes.byref(st)))
                self.first_status = int(st.value)
        if not self._p.value:
            raise FlatGFAError("dev_plan_create", -2)

    def steps_changed(self) -> None:
        """The values of ``graph.steps`` were changed (not the spans): make the plan again from the steps as they are
        (flatgfa_dev_plan_steps_changed; waits for torch's current stream first)."""
        with _torch().cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_plan_steps_changed(self._p, self._stream()), "dev_plan_steps_changed")

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            _lib.lib().flatgfa_dev_plan_destroy(self._p)
            self._p = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> int:
        return _torch().cuda.current_stream(self.graph.device).cuda_stream

    def seg_depth(self, depth_out, uniq_out=None) -> None:
        """Enqueue node depth (+ unique depth when `uniq_out` is given) on torch's current stream.
        Outputs are int32 CUDA tensors of n_segs elements (u32 bits)."""
        torch = _torch()
        S = self.graph.n_segs
        for t in (depth_out, uniq_out):
            if t is not None:
                assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == S
        with torch.cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_seg_depth(self._p, depth_out.data_ptr() if S else None,
                                                    uniq_out.data_ptr() if (uniq_out is not None and S) else None,
                                                    self._stream()), "dev_seg_depth")

    def seg_depth_call(self, depth_out, uniq_out=None, stream=None):
        """A prepared call: returns a function of no arguments that enqueues node depth (+ unique depth) into the given
        tensors on `stream` (a torch.cuda.Stream; None = the stream that is current NOW).  Everything is checked and
        resolved here, once; the function itself is one call through the C ABI -- what a loop that keeps several
        calls in flight wants (the host has 60 us per kernel launch to stay ahead of the device)."""
        torch = _torch()
        S = self.graph.n_segs
        for t in (depth_out, uniq_out):
            if t is not None:
                assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == S
        fn = _lib.lib().flatgfa_dev_seg_depth
        p = self._p
        d = ctypes.c_void_p(depth_out.data_ptr() if S else None)
        u = ctypes.c_void_p(uniq_out.data_ptr() if (uniq_out is not None and S) else None)
        with torch.cuda.device(self.graph.device):
            h = ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.graph.device)).cuda_stream)
        keep = (depth_out, uniq_out, stream)  # (the tensors live as long as the call does)

        def call(_keep=keep):
            rc = fn(p, d, u, h)
            if rc:
                _check(rc, "dev_seg_depth")
        return call

    def path_sums(self, path_ids, depth, length_out, weighted_out) -> None:
        """Enqueue measure_path's integer sums for `path_ids` (int32 CUDA tensor); outputs are
        int64 CUDA tensors (u64 bits)."""
        torch = _torch()
        n = int(path_ids.numel())
        assert path_ids.dtype == torch.int32 and length_out.dtype == torch.int64 and weighted_out.dtype == torch.int64
        assert length_out.numel() == n and weighted_out.numel() == n
        with torch.cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_path_sums(self._p, path_ids.data_ptr() if n else None, n,
                                                    depth.data_ptr() if self.graph.n_segs else None,
                                                    length_out.data_ptr() if n else None,
                                                    weighted_out.data_ptr() if n else None, self._stream()),
                   "dev_path_sums")

    def path_depth_all(self, depth_out, length_out, weighted_out) -> None:
        """Enqueue node depth AND measure_path's two integer sums for every path of the graph
        (what `fgfa depth` needs) in one pass over the steps.  depth_out: int32[n_segs]; the sums:
        int64[n_paths] CUDA tensors (u64 bits), indexed by path."""
        torch = _torch()
        S, P = self.graph.n_segs, self.graph.n_paths
        assert depth_out.dtype == torch.int32 and depth_out.numel() == S and depth_out.is_contiguous()
        for t in (length_out, weighted_out):
            assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == P
        with torch.cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_path_depth_all(self._p, depth_out.data_ptr() if S else None,
                                                         length_out.data_ptr() if P else None,
                                                         weighted_out.data_ptr() if P else None, self._stream()),
                   "dev_path_depth_all")

    def path_overlaps(self, query_ids, touch_out) -> None:
        """Enqueue path-pair overlap (slow_odgi/overlap.py:6-14): touch_out[k * n_paths + j] = 1 iff path
        j touches path query_ids[k].  query_ids: int32[n_q], touch_out: uint8[n_q * n_paths], CUDA tensors."""
        torch = _torch()
        n = int(query_ids.numel())
        assert query_ids.dtype == torch.int32 and touch_out.dtype == torch.uint8 and touch_out.numel() == n * self.graph.n_paths
        with torch.cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_path_overlaps(self._p, query_ids.data_ptr() if n else None, n,
                                                        touch_out.data_ptr() if touch_out.numel() else None,
                                                        self._stream()), "dev_path_overlaps")

    def describe(self) -> str:
        """Which kernels this plan's calls run (the choices made, some by timing, when it was created)."""
        buf = ctypes.create_string_buffer(1024)
        _lib.lib().flatgfa_dev_plan_describe(self._p, buf, 1024)
        return buf.value.decode()

    def status(self) -> None:
        """Synchronize the current stream and raise if a kernel saw an out-of-range id."""
        with _torch().cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_status(self._p, self._stream()), "dev_status")


class DepthPipeline:
    """Calls in flight (flatgfa_dev_pipeline_t): K plans of one resident graph on K internal streams, taken in turn, so
    that pass 2 of one call shares the chip with pass 1 of the next.  `seg_depth` enqueues and returns; the buffers of a
    call may be read after `join()` (torch's current stream then waits for every call so far) or `status()`.
    As with a DepthPlan, the lanes' plans are laid out for the step values they were made with: after writing to
    ``graph.steps`` call :meth:`steps_changed`."""

    def __init__(self, graph: DeviceGraph, calls_in_flight: int = 2):
        torch = _torch()
        self.graph = graph
        self.calls_in_flight = int(calls_in_flight)
        with torch.cuda.device(graph.device):
            g = graph.c_struct()
            self._p = ctypes.c_void_p(_lib.lib().flatgfa_dev_pipeline_create(
                ctypes.byref(g), graph.h_path_begin.ctypes.data if graph.n_paths else None,
                graph.h_path_end.ctypes.data if graph.n_paths else None, self.calls_in_flight))
        if not self._p.value:
            raise FlatGFAError("dev_pipeline_create", -2)

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            _lib.lib().flatgfa_dev_pipeline_destroy(self._p)
            self._p = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seg_depth(self, depth_out, uniq_out=None, after_current_stream: bool = True) -> None:
        """Enqueue node depth (+ unique depth) on the pipeline's next lane.  With `after_current_stream` the call first
        waits for what torch's current stream holds so far (whoever filled the inputs or read these buffers last)."""
        torch = _torch()
        S = self.graph.n_segs
        for t in (depth_out, uniq_out):
            if t is not None:
                assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == S
        with torch.cuda.device(self.graph.device):
            after = ctypes.c_void_p(torch.cuda.current_stream(self.graph.device).cuda_stream) if after_current_stream else ctypes.c_void_p(-1)
            _check(_lib.lib().flatgfa_dev_pipeline_seg_depth(self._p, depth_out.data_ptr() if S else None,
                                                             uniq_out.data_ptr() if (uniq_out is not None and S) else None, after),
                   "dev_pipeline_seg_depth")

    def path_depth_all(self, depth_out, length_out, weighted_out, after_current_stream: bool = True) -> None:
        """Enqueue node depth and measure_path's two sums for every path (what `fgfa depth` needs) on the next lane."""
        torch = _torch()
        S, P = self.graph.n_segs, self.graph.n_paths
        assert depth_out.dtype == torch.int32 and depth_out.numel() == S and depth_out.is_contiguous()
        for t in (length_out, weighted_out):
            assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == P
        with torch.cuda.device(self.graph.device):
            after = ctypes.c_void_p(torch.cuda.current_stream(self.graph.device).cuda_stream) if after_current_stream else ctypes.c_void_p(-1)
            _check(_lib.lib().flatgfa_dev_pipeline_path_depth_all(self._p, depth_out.data_ptr() if S else None, length_out.data_ptr() if P else None,
                                                                  weighted_out.data_ptr() if P else None, after), "dev_pipeline_path_depth_all")

    def steps_changed(self) -> None:
        """The values of ``graph.steps`` were changed: every lane's plan is made again (flatgfa_dev_pipeline_steps_changed)."""
        with _torch().cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_pipeline_steps_changed(self._p), "dev_pipeline_steps_changed")

    def join(self) -> None:
        """torch's current stream waits for every call enqueued so far (no host wait)."""
        torch = _torch()
        with torch.cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_pipeline_join(self._p, ctypes.c_void_p(torch.cuda.current_stream(self.graph.device).cuda_stream)),
                   "dev_pipeline_join")

    def status(self) -> None:
        """Wait for every lane and raise if a kernel saw an out-of-range id."""
        with _torch().cuda.device(self.graph.device):
            _check(_lib.lib().flatgfa_dev_pipeline_status(self._p), "dev_pipeline_status")

    def describe(self) -> str:
        buf = ctypes.create_string_buffer(1024)
        _lib.lib().flatgfa_dev_pipeline_describe(self._p, buf, 1024)
        return buf.value.decode()


def pangenotype_row(gfa, text, row, first_bad, stream=None) -> None:
    """Enqueue one pangenotype row (flatgfa_dev_pangenotype_row): the segments that the whole lines of GAF text in `text`
    (a uint8 CUDA tensor; what follows its last newline is ignored) name are OR-ed into `row` (int64[ceil(S / 64)]: bit
    s & 63 of word s >> 6 is segment s), and a name the graph lacks lowers first_bad[0] (int64; set it to -1, all ones,
    first) to its line's byte offset.  `gfa` is a FlatGFA; `stream` defaults to torch's current stream."""
    torch = _torch()
    S = gfa.segment_count
    assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
    assert row.dtype == torch.int64 and row.is_cuda and row.is_contiguous() and row.numel() == (S + 63) // 64
    assert first_bad.dtype == torch.int64 and first_bad.is_cuda and first_bad.numel() >= 1
    with torch.cuda.device(text.device):
        st = stream if stream is not None else torch.cuda.current_stream(text.device)
        n = int(text.numel())
        _check(_lib.lib().flatgfa_dev_pangenotype_row(gfa._h, text.data_ptr() if n else None, n, row.data_ptr() if row.numel() else None,
                                                      first_bad.data_ptr(), ctypes.c_void_p(st.cuda_stream)), "dev_pangenotype_row")


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _expand(graph: DeviceGraph, what: str, stream, count, n_added: int = 0):
    """What chop and inject share: `count(L, g, seg_first, stream, job, n_segs, n_steps)` calls flatgfa_dev_<what>_count
    with the feature's own arguments beside these and returns its code; the image of graph.n_paths + n_added paths is then
    allocated and filled, and the job freed.  Returns (the new DeviceGraph, seg_first)."""
    torch = _torch()
    if graph.seg_len is None:
        raise FlatGFAError(what + ": the graph has no seg_len", -1)
    with torch.cuda.device(graph.device):
        st = stream if stream is not None else torch.cuda.current_stream(graph.device)
        st_ptr = ctypes.c_void_p(st.cuda_stream)
        g = graph.c_struct()
        seg_first = torch.empty(graph.n_segs + 1, dtype=torch.int32, device=graph.device)
        job = ctypes.c_void_p()
        n_segs, n_steps = ctypes.c_uint64(), ctypes.c_uint64()
        L = _lib.lib()
        _check(count(L, ctypes.byref(g), seg_first.data_ptr(), st_ptr, ctypes.byref(job), ctypes.byref(n_segs), ctypes.byref(n_steps)),
               "dev_%s_count" % what)
        try:
            steps = torch.empty(n_steps.value, dtype=torch.int32, device=graph.device)
            pb = torch.empty(graph.n_paths + n_added, dtype=torch.int32, device=graph.device)
            pe = torch.empty(graph.n_paths + n_added, dtype=torch.int32, device=graph.device)
            seg_len = torch.empty(n_segs.value, dtype=torch.int32, device=graph.device)
            _check(getattr(L, "flatgfa_dev_%s_fill" % what)(job, _ptr(steps), _ptr(pb), _ptr(pe), _ptr(seg_len), st_ptr), "dev_%s_fill" % what)
        finally:
            getattr(L, "flatgfa_dev_%s_free" % what)(job)  # (waits for the fill)
        return DeviceGraph.from_tensors(steps, pb, pe, n_segs.value, seg_len), seg_first


def chop(graph: DeviceGraph, max_size: int, stream=None) -> Tuple[DeviceGraph, object]:
    """chop (flatgfa/src/ops/chop.rs, without links) of a resident graph image, on the device: returns the chopped image
    as a new DeviceGraph (int32 tensors on the same device; a valid input to DepthPlan) and seg_first (int32[n_segs + 1]:
    old segment s became the new segments [seg_first[s], seg_first[s + 1])).  Needs graph.seg_len.  Waits for the stream
    once, to learn the sizes (flatgfa_dev_chop_count); the rest is enqueued on it (torch's current stream by default)."""
    return _expand(graph, "chop", stream, lambda L, g, seg_first, st, job, n_segs, n_steps:
                   L.flatgfa_dev_chop_count(g, int(max_size), seg_first, st, job, n_segs, n_steps))


def inject(graph: DeviceGraph, path_ids, starts, ends, stream=None) -> Tuple[DeviceGraph, object]:
    """inject (slow_odgi/inject.py, without links or names) of a resident graph image, on the device: line l is bases
    [starts[l], ends[l]) of path path_ids[l] (int32 / int64 / int64 CUDA tensors of one length).  Returns the new image as a
    DeviceGraph -- the old paths, cut, then one new path per line; a valid input to DepthPlan -- and seg_first
    (int32[n_segs + 1]: old segment s became the new segments [seg_first[s], seg_first[s + 1])).  Needs graph.seg_len.  Waits
    for the stream once, to learn the sizes (flatgfa_dev_inject_count); the rest is enqueued on it (torch's current stream by
    default)."""
    torch = _torch()
    if graph.seg_len is None:
        raise FlatGFAError("inject: the graph has no seg_len", -1)
    n = int(path_ids.numel())
    assert path_ids.dtype == torch.int32 and starts.dtype == torch.int64 and ends.dtype == torch.int64
    assert starts.numel() == n and ends.numel() == n
    assert all(t.is_cuda and t.is_contiguous() for t in (path_ids, starts, ends))
    n_paths = ctypes.c_uint64()  # (graph.n_paths + n)
    return _expand(graph, "inject", stream, lambda L, g, seg_first, st, job, n_segs, n_steps:
                   L.flatgfa_dev_inject_count(g, _ptr(path_ids), _ptr(starts), _ptr(ends), n, seg_first, st, job, n_segs, n_steps,
                                              ctypes.byref(n_paths)), n)


def crush(graph: DeviceGraph, seg_seq, seq_data, stream=None):
    """crush (slow_odgi/crush.py) of a resident graph image and its sequence pool, on the device: seg_seq is int32[2 * n_segs]
    (each segment's start in seq_data and its length, as the GAF lookup keeps them), seq_data the pool (uint8), both CUDA
    tensors.  Returns (the crushed image, seq_out, seg_seq_out): a DeviceGraph that shares graph's step and span tensors and
    has the new lengths as seg_len (a valid input to DepthPlan), the new pool (uint8: the crushed segments in segment order)
    and the new spans (int32[2 * n_segs]).  Waits for the stream once, to learn the sizes (flatgfa_dev_crush_count); the rest
    is enqueued on it (torch's current stream by default)."""
    torch = _torch()
    S = graph.n_segs
    assert seg_seq.dtype == torch.int32 and seg_seq.is_cuda and seg_seq.is_contiguous() and seg_seq.numel() == 2 * S
    assert seq_data.dtype == torch.uint8 and seq_data.is_cuda and seq_data.is_contiguous()
    with torch.cuda.device(graph.device):
        st = stream if stream is not None else torch.cuda.current_stream(graph.device)
        seg_len = torch.empty(S, dtype=torch.int32, device=graph.device)
        job = ctypes.c_void_p()
        kept, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        L = _lib.lib()

        def ptr(t):
            return t.data_ptr() if t.numel() else None
        with torch.cuda.stream(st):  # (the outputs are the stream's: torch's allocator may hand their memory on behind it)
            _check(L.flatgfa_dev_crush_count(ptr(seg_seq), ptr(seq_data), int(seq_data.numel()), S, ptr(seg_len),
                                             ctypes.c_void_p(st.cuda_stream), ctypes.byref(job), ctypes.byref(kept), ctypes.byref(dropped)),
                   "dev_crush_count")
            try:
                seq_out = torch.empty(kept.value, dtype=torch.uint8, device=graph.device)
                seg_seq_out = torch.empty(2 * S, dtype=torch.int32, device=graph.device)
                _check(L.flatgfa_dev_crush_fill(job, ptr(seq_out), ptr(seg_seq_out), ctypes.c_void_p(st.cuda_stream)), "dev_crush_fill")
            finally:
                L.flatgfa_dev_crush_free(job)  # (waits for the fill, on this stream only)
        new = DeviceGraph.from_tensors(graph.steps, graph.path_begin, graph.path_end, S, seg_len, graph.h_path_begin, graph.h_path_end)
        return new, seq_out, seg_seq_out


def flip(graph: DeviceGraph, links, stream=None, alignment=None, round_keys: int = 0):
    """flip (slow_odgi/flip.py) of a resident graph image and its links, on the device: links is int32[4 * n_links], the
    Link records (from, to, overlap.start, overlap.end), and alignment the int32 pool their overlaps point into (None: an
    empty pool, for links whose overlap spans are all empty), both CUDA tensors.  Returns (the flipped image, links_out,
    turned): a DeviceGraph whose steps are the paths one behind another in path order -- the turned ones reversed, every
    orientation toggled -- and which shares graph's seg_len (a valid input to DepthPlan); the kept Link records (int32[4 *
    n]: the old links without their duplicates, then the new ones, whose overlap [len(alignment), len(alignment) + 1) is
    the one 0M op, the word 0, that the caller appends to its pool); and the turned flags (int32[n_paths], 0 or 1).  Needs
    graph.seg_len.  round_keys (0: the library's 2^26) is for tests and measurements: how many keys of the link table a round
    of the grouping takes; it never changes the answer.  Waits for the stream once, to learn the sizes (flatgfa_dev_flip_count); the rest is enqueued on it
    (torch's current stream by default)."""
    torch = _torch()
    if graph.seg_len is None:
        raise FlatGFAError("flip: the graph has no seg_len", -1)
    assert links.dtype == torch.int32 and links.is_cuda and links.is_contiguous() and links.numel() % 4 == 0
    if alignment is not None:
        assert alignment.dtype == torch.int32 and alignment.is_cuda and alignment.is_contiguous()
    P = graph.n_paths
    lens = graph.h_path_end.astype(np.int64) - graph.h_path_begin.astype(np.int64)
    if (lens < 0).any() or int(lens.sum()) > 0xFFFFFFFF:
        raise FlatGFAError("flip: a path span ends before it begins, or the paths hold more than 2^32 - 1 steps", -2)
    h_start = np.zeros(P + 1, dtype=np.uint32)
    h_start[1:] = np.cumsum(lens, dtype=np.int64).astype(np.uint32)
    n_lin = int(h_start[P])
    with torch.cuda.device(graph.device):
        st = stream if stream is not None else torch.cuda.current_stream(graph.device)
        st_ptr = ctypes.c_void_p(st.cuda_stream)
        job = ctypes.c_void_p()
        n_turned, n_out, n_new = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        L = _lib.lib()
        n_align = 0 if alignment is None else int(alignment.numel())
        with torch.cuda.stream(st):  # (the outputs are the stream's: torch's allocator may hand their memory on behind it)
            start = _as_i32(h_start).to(graph.device)
            _check(L.flatgfa_dev_flip_count(_ptr(graph.steps), graph.n_steps, start.data_ptr(), _ptr(graph.path_begin), P, n_lin,
                                            _ptr(graph.seg_len), graph.n_segs, _ptr(links), int(links.numel()) // 4,
                                            None if alignment is None else _ptr(alignment), n_align, int(round_keys), st_ptr, ctypes.byref(job),
                                            ctypes.byref(n_turned), ctypes.byref(n_out), ctypes.byref(n_new)), "dev_flip_count")
            try:
                steps = torch.empty(n_lin, dtype=torch.int32, device=graph.device)
                turned = torch.empty(P, dtype=torch.int32, device=graph.device)
                links_out = torch.empty(4 * n_out.value, dtype=torch.int32, device=graph.device)
                _check(L.flatgfa_dev_flip_fill(job, _ptr(steps), _ptr(turned), _ptr(links_out), st_ptr), "dev_flip_fill")
            finally:
                L.flatgfa_dev_flip_free(job)  # (waits for the fill, on this stream only)
            new = DeviceGraph.from_tensors(steps, start[:P].contiguous(), start[1:].contiguous(), graph.n_segs, graph.seg_len, h_start[:P], h_start[1:])
        return new, links_out, turned


def seq_pack(text, stream=None, carry: int = -1):
    """The packed-sequence codec's pack (packedseq.rs) of nucleotide text on the device: text is a uint8 CUDA tensor, at any
    alignment (a slice will do).  Returns (packed, n_bases): a uint8 tensor of (n_bases + (carry >= 0) + 1) // 2 bytes -- two
    bases a byte, A 0, C 1, T 2, G 3, the even base in the low nibble -- and the number of bases kept.  Whitespace is dropped;
    another byte that is not one of A C T G raises FlatGFAError (code -7) naming the smallest offending offset.  carry: a code
    0..3 that goes in front of the bases (what a caller that cuts its text in pieces held back from the piece before), or -1.
    Waits for the stream once, to learn the count (flatgfa_dev_seq_pack_count); the rest is enqueued on it (torch's current
    stream by default)."""
    torch = _torch()
    assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
    with torch.cuda.device(text.device):
        st = stream if stream is not None else torch.cuda.current_stream(text.device)
        job, kept = ctypes.c_void_p(), ctypes.c_uint64()
        L = _lib.lib()
        with torch.cuda.stream(st):  # (the output is the stream's: torch's allocator may hand its memory on behind it)
            _check(L.flatgfa_dev_seq_pack_count(_ptr(text), int(text.numel()), ctypes.c_void_p(st.cuda_stream), ctypes.byref(job), ctypes.byref(kept)),
                   "dev_seq_pack_count")
            try:
                packed = torch.empty((kept.value + (1 if carry >= 0 else 0) + 1) // 2, dtype=torch.uint8, device=text.device)
                _check(L.flatgfa_dev_seq_pack_fill(job, int(carry), _ptr(packed), ctypes.c_void_p(st.cuda_stream)), "dev_seq_pack_fill")
            finally:
                L.flatgfa_dev_seq_pack_free(job)  # (waits for the fill, on this stream only)
        return packed, kept.value


def seq_unpack(packed, n_bases: int, stream=None):
    """The letters of the first n_bases nibbles of `packed` (a uint8 CUDA tensor of at least (n_bases + 1) // 2 bytes) as a
    uint8 tensor, on the device.  A nibble above 3 among them raises FlatGFAError (code -7) naming the smallest such base
    index; the unused high nibble of an odd count's last byte is not looked at.  Waits for the stream once, for that answer."""
    torch = _torch()
    assert packed.dtype == torch.uint8 and packed.is_cuda and packed.is_contiguous() and packed.numel() >= (n_bases + 1) // 2
    with torch.cuda.device(packed.device):
        st = stream if stream is not None else torch.cuda.current_stream(packed.device)
        with torch.cuda.stream(st):
            text = torch.empty(n_bases, dtype=torch.uint8, device=packed.device)
            _check(_lib.lib().flatgfa_dev_seq_unpack(_ptr(packed), int(n_bases), _ptr(text), ctypes.c_void_p(st.cuda_stream)), "dev_seq_unpack")
        return text


BED_ROUND_CANDS = 1 << 22  # kBedRoundCands (csrc/bed_device.hpp)


def bed_intersect(a_ids, a_start, a_end, b_ids, b_start, b_end, n_groups=None, stream=None, round_cands: int = BED_ROUND_CANDS):
    """BED intersection (pollen_amd.bed_intersect, without names or text) of entries on the device.  Entry i of a side has the
    name id ids[i] (int32 CUDA tensor) and the interval [start[i], end[i]) (int64 CUDA tensors, read as u64).  b is grouped:
    its ids never decrease and lie below n_groups (by default the last id + 1), file order kept inside a group; a's ids lie
    below n_groups, or are -1 for a name b does not have.  Returns (a_index, b_index, start, end): one record per hit in the
    reference's order -- a entry after a entry, inside one in b's order -- with start = the max of the two starts and end =
    the min of the two ends.  The hits are found round_cands candidate pairs at a time, into scratch of that size.  Waits for
    the stream once per round."""
    torch = _torch()
    for t in (a_ids, b_ids):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    for t in (a_start, a_end, b_start, b_end):
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous()
    n_a, n_b = int(a_ids.numel()), int(b_ids.numel())
    assert a_start.numel() == a_end.numel() == n_a and b_start.numel() == b_end.numel() == n_b and round_cands >= 1
    dev = a_ids.device
    with torch.cuda.device(dev):
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if n_groups is None:
            n_groups = int(b_ids[-1].item()) + 1 if n_b else 0
        L = _lib.lib()
        job = ctypes.c_void_p()
        cands, rounds, unsorted = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        parts = []
        with torch.cuda.stream(st):  # (the outputs are the stream's: torch's allocator may hand their memory on behind it)
            _check(L.flatgfa_dev_bed_begin(_ptr(a_ids), _ptr(a_start), _ptr(a_end), n_a, _ptr(b_ids), _ptr(b_start), _ptr(b_end), n_b,
                                           int(n_groups), int(round_cands), ctypes.c_void_p(st.cuda_stream), ctypes.byref(job),
                                           ctypes.byref(cands), ctypes.byref(rounds), ctypes.byref(unsorted)), "dev_bed_begin")
            try:
                room = min(cands.value, int(round_cands))
                ai = torch.empty(room, dtype=torch.int32, device=dev)
                bi = torch.empty(room, dtype=torch.int32, device=dev)
                s = torch.empty(room, dtype=torch.int64, device=dev)
                e = torch.empty(room, dtype=torch.int64, device=dev)
                for r in range(rounds.value):
                    n = ctypes.c_uint64()
                    _check(L.flatgfa_dev_bed_round(job, r, _ptr(ai), _ptr(bi), _ptr(s), _ptr(e), ctypes.byref(n)), "dev_bed_round")
                    parts.append(tuple(t[:n.value].clone() for t in (ai, bi, s, e)))
            finally:
                L.flatgfa_dev_bed_free(job)
            if not parts:
                parts.append((torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                              torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)))
            return tuple(torch.cat([p[k] for p in parts]) for k in range(4))


def profile_enable(on: bool) -> None:
    _lib.lib().flatgfa_dev_profile_enable(1 if on else 0)


def profile_overhead_ms(n_workgroups: int = 256, lds_bytes: int = 142 * 1024, reps: int = 20) -> float:
    """What the event pair of a profiled kernel reads around a launch that does nothing."""
    import torch
    return float(_lib.lib().flatgfa_dev_profile_overhead_ms(n_workgroups, lds_bytes, reps, torch.cuda.current_stream().cuda_stream))


def profile_read(cap: int = 4096) -> List[Tuple[str, float]]:
    names = (ctypes.c_char_p * cap)()
    ms = (ctypes.c_float * cap)()
    n = _lib.lib().flatgfa_dev_profile_read(names, ms, cap)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]
