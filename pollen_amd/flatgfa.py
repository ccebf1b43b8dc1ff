"""Host-side mirror of the reference's FlatGFA interface for the depth path, over the C ABI.

Names and argument meaning follow the reference (cucapra/pollen):
  parse / parse_bytes / load / write_flatgfa / write_gfa      flatgfa-py/flatgfa.pyi:80-93
  seg_depth / seg_depth_with_uniq / path_depth                flatgfa/src/ops/depth.rs:15,45,88
  depth_table / path_depth_table  (`fgfa depth [-d] [-r P]`)  flatgfa/src/cli/cmds.rs:234-285

Every depth method runs the HIP kernels in libflatgfa.so; there is no Python or CPU
implementation of them in this package.
"""
from __future__ import annotations

import ctypes
import mmap
import os
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import flatgfa_handle_t

# Packed reference layouts (flatgfa.rs:71-82, 99-112, 121-133; pool.rs:80-86).
SEG_DT = np.dtype([("name", "<u8"), ("seq_start", "<u4"), ("seq_end", "<u4"),
                   ("opt_start", "<u4"), ("opt_end", "<u4")])
PATH_DT = np.dtype([("name_start", "<u4"), ("name_end", "<u4"), ("steps_start", "<u4"),
                    ("steps_end", "<u4"), ("ov_start", "<u4"), ("ov_end", "<u4")])
LINK_DT = np.dtype([("from_", "<u4"), ("to", "<u4"), ("ov_start", "<u4"), ("ov_end", "<u4")])
SPAN_DT = np.dtype([("start", "<u4"), ("end", "<u4")])
POOLS = ["header", "segs", "paths", "links", "steps", "seq_data", "overlaps", "alignment",
         "name_data", "optional_data", "line_order"]
_POOL_DT = {"header": np.dtype("u1"), "segs": SEG_DT, "paths": PATH_DT, "links": LINK_DT,
            "steps": np.dtype("<u4"), "seq_data": np.dtype("u1"), "overlaps": SPAN_DT,
            "alignment": np.dtype("<u4"), "name_data": np.dtype("u1"),
            "optional_data": np.dtype("u1"), "line_order": np.dtype("u1")}

ERR_BOUNDS = -2
ERR_NO_DEVICE = -3


class FlatGFAError(RuntimeError):
    def __init__(self, what: str, code: int = 0):
        super().__init__(f"{what}: {_lib.last_error()}" + (f" (code {code})" if code else ""))
        self.code = code


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise FlatGFAError(what, rc)


def _take_text(ptr: ctypes.c_void_p, n: ctypes.c_size_t) -> bytes:
    out = bytes((ctypes.c_char * n.value).from_address(ptr.value)) if ptr.value and n.value else b""  # (string_at takes a C int)
    _lib.lib().flatgfa_free_text(ptr)
    return out


class FlatGFA:
    """An owned graph handle (`flatgfa_t`).  Freed on garbage collection or `close()`."""

    def __init__(self, handle: int):
        if not handle:
            raise FlatGFAError("cannot create FlatGFA")
        self._h = ctypes.c_void_p(handle)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().flatgfa_free(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "FlatGFA":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # ---- flatgfa-py style list views (flatgfa-py/flatgfa.pyi:80-88) ----
    def _views(self):
        from . import views
        if getattr(self, "_pools_cache", None) is None:
            self._pools_cache = views._Pools(self)
        return views, self._pools_cache

    @property
    def segments(self):
        v, p = self._views()
        return v.SegmentList(p)

    @property
    def paths(self):
        v, p = self._views()
        return v.PathList(p)

    @property
    def links(self):
        v, p = self._views()
        return v.LinkList(p)

    # ---- flatgfa-c accessors (flatgfa-c/src/lib.rs:80-172) ----
    @property
    def segment_count(self) -> int:
        return _lib.lib().flatgfa_get_segment_count(self._h)

    @property
    def path_count(self) -> int:
        return _lib.lib().flatgfa_path_count(self._h)

    def get_seq(self, segment_id: int) -> Optional[bytes]:
        s = _lib.lib().flatgfa_get_seq(self._h, segment_id)
        if segment_id >= self.segment_count:
            assert not s.data and s.len == 0
            return None
        return ctypes.string_at(s.data, s.len)

    def get_path_name(self, path_index: int) -> Optional[bytes]:
        if path_index >= self.path_count:
            s = _lib.lib().flatgfa_get_path_name(self._h, path_index)
            assert not s.data and s.len == 0
            return None
        s = _lib.lib().flatgfa_get_path_name(self._h, path_index)
        return ctypes.string_at(s.data, s.len)

    def get_path_step_count(self, path_index: int) -> int:
        return _lib.lib().flatgfa_get_path_step_count(self._h, path_index)

    def get_step(self, path_index: int, step_index: int) -> Optional[Tuple[int, bool]]:
        out = flatgfa_handle_t()
        ok = _lib.lib().flatgfa_get_step(self._h, path_index, step_index, ctypes.byref(out))
        return (out.segment_id, bool(out.is_forward)) if ok else None

    def find_path(self, name: bytes) -> Optional[int]:
        i = _lib.lib().flatgfa_find_path(self._h, name, len(name))
        return None if i < 0 else int(i)

    # ---- pools ----
    def pool(self, name: str) -> np.ndarray:
        """A copy of one pool as a numpy array in the reference's packed layout."""
        ix = POOLS.index(name)
        data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.lib().flatgfa_pool(self._h, ix, ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)), "pool")
        dt = _POOL_DT[name]
        assert dt.itemsize == es.value
        if n.value == 0:
            return np.zeros(0, dtype=dt)
        # (ctypes.string_at takes a C int: pools beyond 2 GiB would be cut short)
        raw = (ctypes.c_char * (n.value * es.value)).from_address(data.value)
        return np.frombuffer(raw, dtype=dt).copy()

    def soa(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The structure-of-arrays image the kernels read: (steps, path_begin, path_end, seg_len)."""
        paths, segs = self.pool("paths"), self.pool("segs")
        return (self.pool("steps"), np.ascontiguousarray(paths["steps_start"]),
                np.ascontiguousarray(paths["steps_end"]),
                (segs["seq_end"] - segs["seq_start"]).astype(np.uint32))

    # ---- writers (flatgfa-py: write_flatgfa / write_gfa / str) ----
    def write_flatgfa(self, filename: str) -> None:
        _check(_lib.lib().flatgfa_write_flatgfa(self._h, os.fsencode(filename)), "write_flatgfa")

    def write_flatgfa_prealloc(self, filename: str, gfa_text: Optional[bytes] = None, factor: int = 32) -> None:
        """The preallocated container of `fgfa -m -p FACTOR -o OUT [-I GFA]` (cli/main.rs:216-248):
        capacities estimated from `gfa_text` (the text this graph was parsed from), or guessed from `factor`."""
        _check(_lib.lib().flatgfa_write_flatgfa_prealloc(self._h, os.fsencode(filename), gfa_text, len(gfa_text) if gfa_text is not None else 0,
                                                         int(factor)), "write_flatgfa_prealloc")

    def gfa_text(self) -> bytes:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_print_gfa(self._h, ctypes.byref(p), ctypes.byref(n)), "print_gfa")
        return _take_text(p, n)

    def write_gfa(self, filename: str) -> None:
        with open(filename, "wb") as f:
            f.write(self.gfa_text())

    def __str__(self) -> str:
        return self.gfa_text().decode(errors="replace")

    # ---- the same text, formatted on the GPU (print.rs:99-153; no CPU fallback: gfa_text is that route) ----
    def gfa_bytes(self) -> int:
        """How many bytes the GFA text has (flatgfa_print_gfa_bytes): everything checked and counted, nothing delivered."""
        n = ctypes.c_uint64()
        _check(_lib.lib().flatgfa_print_gfa_bytes(self._h, ctypes.byref(n)), "print_gfa_bytes")
        return int(n.value)

    def gfa_text_device(self) -> bytes:
        """The bytes of gfa_text(), formatted on the GPU (flatgfa_print_gfa_device)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_print_gfa_device(self._h, ctypes.byref(p), ctypes.byref(n)), "print_gfa_device")
        return _take_text(p, n)

    def gfa_stream(self, write) -> None:
        """flatgfa_print_gfa_stream: `write(bytes)` receives the text of gfa_text() in order, a piece at a time.  A `write`
        that raises, or returns something true, stops the call."""
        raised = []

        def sink(_ctx, ptr, n):
            try:
                return 1 if write(ctypes.string_at(ptr, n)) else 0  # (a piece is a few megabytes: within string_at's C int)
            except BaseException as e:  # noqa: BLE001  (must not unwind through the C caller)
                raised.append(e)
                return 1
        rc = _lib.lib().flatgfa_print_gfa_stream(self._h, _lib.SINK_T(sink), None)
        if raised:
            raise raised[0]
        _check(rc, "print_gfa_stream")

    def write_gfa_device(self, filename: str) -> None:
        """write_gfa through the GPU printer, written as it streams.  The file is made once the text has been checked."""
        f = []

        def write(b):
            if not f:
                f.append(open(filename, "wb"))
            f[0].write(b)
        try:
            self.gfa_stream(write)
            if not f:
                f.append(open(filename, "wb"))  # (an empty graph: an empty file)
        finally:
            if f:
                f[0].close()

    # ---- depth queries (HIP) ----
    def to_device(self, device: int = 0) -> None:
        _check(_lib.lib().flatgfa_to_device(self._h, device), "to_device")

    def residency_ms(self) -> Tuple[float, float]:
        """(host-to-device copies, plan creation) of to_device on this handle, milliseconds."""
        h2d, plan = ctypes.c_double(0), ctypes.c_double(0)
        _check(_lib.lib().flatgfa_residency_ms(self._h, ctypes.byref(h2d), ctypes.byref(plan)), "residency_ms")
        return h2d.value, plan.value

    def seg_depth_with_uniq(self) -> Tuple[np.ndarray, np.ndarray]:
        """ops/depth.rs:15-39 -> (depths, uniq_depths), uint64, indexed by segment id."""
        S = self.segment_count
        d, u = np.zeros(S, np.uint64), np.zeros(S, np.uint64)
        _check(_lib.lib().flatgfa_seg_depth(self._h, d.ctypes.data, u.ctypes.data), "seg_depth_with_uniq")
        return d, u

    def seg_depth(self) -> np.ndarray:
        """ops/depth.rs:45-56"""
        d = np.zeros(self.segment_count, np.uint64)
        _check(_lib.lib().flatgfa_seg_depth(self._h, d.ctypes.data, None), "seg_depth")
        return d

    def path_depth(self, path_ids: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """ops/depth.rs:88-111 -> (path_lengths uint64, mean depths float64) for `path_ids`
        (default: all paths, in order)."""
        ids = np.arange(self.path_count, dtype=np.uint32) if path_ids is None \
            else np.ascontiguousarray(path_ids, dtype=np.uint32)
        ln, mean = np.zeros(len(ids), np.uint64), np.zeros(len(ids), np.float64)
        _check(_lib.lib().flatgfa_path_depth(self._h, ids.ctypes.data, len(ids), ln.ctypes.data, mean.ctypes.data),
               "path_depth")
        return ln, mean

    def depth_table(self) -> bytes:
        """The bytes `fgfa depth -d` prints."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_depth_table(self._h, ctypes.byref(p), ctypes.byref(n)), "depth_table")
        return _take_text(p, n)

    def path_depth_table(self, names: Optional[Iterable[bytes]] = None) -> bytes:
        """The bytes `fgfa depth [-r NAME]...` prints; unknown names are dropped (cmds.rs:270-274)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        if names is None:
            rc = _lib.lib().flatgfa_path_depth_table(self._h, None, 0, ctypes.byref(p), ctypes.byref(n))
        else:
            found = [self.find_path(nm) for nm in names]
            ids = np.array([i for i in found if i is not None] + [0], dtype=np.uint32)
            rc = _lib.lib().flatgfa_path_depth_table(self._h, ids.ctypes.data, len(ids) - 1, ctypes.byref(p),
                                                     ctypes.byref(n))
        _check(rc, "path_depth_table")
        return _take_text(p, n)

    def path_depth_bed(self, names: Optional[Iterable[bytes]] = None) -> bytes:
        """PathDepth::as_bed (depth.rs:173-183) as three-column BED text: `name\\t0\\tlength` per path."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        if names is None:
            rc = _lib.lib().flatgfa_path_depth_bed(self._h, None, 0, ctypes.byref(p), ctypes.byref(n))
        else:
            found = [self.find_path(nm) for nm in names]
            ids = np.array([i for i in found if i is not None] + [0], dtype=np.uint32)
            rc = _lib.lib().flatgfa_path_depth_bed(self._h, ids.ctypes.data, len(ids) - 1, ctypes.byref(p), ctypes.byref(n))
        _check(rc, "path_depth_bed")
        return _take_text(p, n)


    # ---- the rows next to the depth path ----
    def _ids(self, paths) -> np.ndarray:
        """Path ids from a list of ids or names; unknown names raise (slow_odgi asserts, overlap.py:21)."""
        out = []
        for p in paths:
            if isinstance(p, (bytes, bytearray)):
                i = self.find_path(bytes(p))
                if i is None:
                    raise FlatGFAError(f"path {bytes(p)!r} not found")
                out.append(i)
            else:
                out.append(int(p))
        return np.ascontiguousarray(out, dtype=np.uint32)

    def seg_depth_subset(self, paths) -> Tuple[np.ndarray, np.ndarray]:
        """Node depth counting only `paths` (`odgi depth -d -s`, slow_odgi/depth.py:12)."""
        ids = self._ids(paths)
        S = self.segment_count
        d, u = np.zeros(S, np.uint64), np.zeros(S, np.uint64)
        _check(_lib.lib().flatgfa_seg_depth_subset(self._h, ids.ctypes.data if len(ids) else None, len(ids),
                                                   d.ctypes.data, u.ctypes.data), "seg_depth_subset")
        return d, u

    def path_overlaps(self, queries) -> np.ndarray:
        """touch[k, j] = path j touches query k (slow_odgi/overlap.py:6-14)."""
        ids = self._ids(queries)
        t = np.zeros((len(ids), self.path_count), np.uint8)
        _check(_lib.lib().flatgfa_path_overlaps(self._h, ids.ctypes.data if len(ids) else None, len(ids),
                                                t.ctypes.data if t.size else None), "path_overlaps")
        return t

    def overlap_table(self, queries) -> bytes:
        """The bytes `slow_odgi overlap --paths FILE` prints."""
        ids = self._ids(queries)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_overlap_table(self._h, ids.ctypes.data if len(ids) else None, len(ids),
                                                ctypes.byref(p), ctypes.byref(n)), "overlap_table")
        return _take_text(p, n)

    def interval_depth(self, path, starts, ends) -> np.ndarray:
        """ops/window_depth.rs:176-180"""
        (pid,) = self._ids([path])
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        en = np.ascontiguousarray(ends, dtype=np.uint64)
        out = np.zeros(len(st), np.float64)
        _check(_lib.lib().flatgfa_interval_depth(self._h, int(pid), st.ctypes.data, en.ctypes.data, len(st),
                                                 out.ctypes.data), "interval_depth")
        return out

    def window_depth_table(self, path, window: int) -> bytes:
        """The bytes `fgfa window-depth PATH SIZE` prints."""
        (pid,) = self._ids([path])
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_window_depth_table(self._h, int(pid), window, ctypes.byref(p), ctypes.byref(n)),
               "window_depth_table")
        return _take_text(p, n)

    def bed_depth_table(self, bed: bytes) -> bytes:
        """The bytes `fgfa depth -b FILE.bed` prints."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_bed_depth_table(self._h, bed, len(bed), ctypes.byref(p), ctypes.byref(n)),
               "bed_depth_table")
        return _take_text(p, n)

    def intervals_depth(self, paths, starts, ends) -> np.ndarray:
        """Interval k lies on paths[k] (names or ids); every maximal run of one path is one interval_depth of the reference
        (ops/window_depth.rs:116-147).  The walk runs on the GPU; only the float64 results come back."""
        ids = self._ids(paths)
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        en = np.ascontiguousarray(ends, dtype=np.uint64)
        if not len(ids) == len(st) == len(en):
            raise FlatGFAError("intervals_depth: paths, starts and ends differ in length")
        out = np.zeros(len(st), np.float64)
        _check(_lib.lib().flatgfa_intervals_depth(self._h, ids.ctypes.data, st.ctypes.data, en.ctypes.data, len(st),
                                                  out.ctypes.data), "intervals_depth")
        return out

    def window_depth_paths_table(self, window: int, paths=None) -> bytes:
        """The bytes `fgfa window-depth-all SIZE` prints: `fgfa window-depth P SIZE` for every path (or the listed ones), in order."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        if paths is None:
            rc = _lib.lib().flatgfa_window_depth_paths_table(self._h, None, 0, window, ctypes.byref(p), ctypes.byref(n))
        else:
            ids = self._ids(paths)
            rc = _lib.lib().flatgfa_window_depth_paths_table(self._h, ids.ctypes.data, len(ids), window, ctypes.byref(p), ctypes.byref(n))
        _check(rc, "window_depth_paths_table")
        return _take_text(p, n)

    def bed_depth_paths_table(self, bed: bytes) -> bytes:
        """The bytes `fgfa depth --bed-paths FILE.bed` prints: every entry on the path it names."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_bed_depth_paths_table(self._h, bed, len(bed), ctypes.byref(p), ctypes.byref(n)),
               "bed_depth_paths_table")
        return _take_text(p, n)

    def _gaf_call(self, gafs, call):
        """`call(ptrs, lens, n)` over GAF texts: file names are mapped (never read into Python), bytes-likes passed as they are."""
        maps, arrs = [], []
        try:
            for g in gafs:
                if isinstance(g, (bytes, bytearray, memoryview)):
                    arrs.append(np.frombuffer(g, dtype=np.uint8))
                    continue
                with open(g, "rb") as f:
                    size = os.fstat(f.fileno()).st_size
                    if size == 0:  # (mmap cannot map an empty file)
                        arrs.append(np.zeros(0, dtype=np.uint8))
                        continue
                    m = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                maps.append(m)
                arrs.append(np.frombuffer(m, dtype=np.uint8))
            n = len(arrs)
            ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
            lens = (ctypes.c_size_t * max(n, 1))(*[a.size for a in arrs])
            return call(ptrs, lens, n)
        finally:
            arrs.clear()
            for m in maps:
                try:
                    m.close()
                except BufferError:  # (a view of it is still alive somewhere: the mapping goes with it)
                    pass

    def pangenotype_matrix(self, gafs) -> np.ndarray:
        """bool[len(gafs), segment_count]: which segments some alignment of each GAF names in its path field
        (flatgfa/src/ops/pangenotype.rs:11-70).  `gafs`: file names or bytes, one per row."""
        gafs = list(gafs)
        S = self.segment_count
        W = (S + 63) // 64
        bits = np.zeros((len(gafs), W), dtype=np.uint64)
        self._gaf_call(gafs, lambda p, l, n: _check(
            _lib.lib().flatgfa_pangenotype_matrix(self._h, p, l, n, bits.ctypes.data if bits.size else None), "pangenotype_matrix"))
        return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :S].astype(bool)

    def make_pangenotype_matrix(self, gaf_files: Sequence[str]) -> List[List[bool]]:
        """flatgfa-py's FlatGFA.make_pangenotype_matrix (flatgfa.pyi:89): one list of bools per GAF file."""
        return self.pangenotype_matrix(gaf_files).tolist()

    def pangenotype_table(self, gafs) -> bytes:
        """The bytes `fgfa matrix GAF` prints (cli/cmds.rs:465-474), a line per item of `gafs`."""
        gafs = list(gafs)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._gaf_call(gafs, lambda ptrs, lens, k: _check(
            _lib.lib().flatgfa_pangenotype_table(self._h, ptrs, lens, k, ctypes.byref(p), ctypes.byref(n)), "pangenotype_table"))
        return _take_text(p, n)

    # ---- GAF lookup (ops/gaf.rs) ----
    def _gaf_text(self, gaf, call):
        """`call(pointer, length, array)` over one GAF text: a file name (mapped) or bytes."""
        box = []
        self._gaf_call([gaf], lambda ptrs, lens, n: box.append(call(ptrs[0], lens[0])))
        return box[0]

    def gaf_count(self, gaf) -> int:
        """`fgfa gaf GAF -b`: the number of events of all reads (flatgfa/src/cli/cmds.rs:325-347)."""
        ev = ctypes.c_uint64()
        self._gaf_text(gaf, lambda p, n: _check(_lib.lib().flatgfa_gaf_count(self._h, p, n, ctypes.byref(ev), None), "gaf_count"))
        return int(ev.value)

    def gaf_seqs(self, gaf) -> bytes:
        """The bytes `fgfa gaf GAF -s` prints: per read its name, a tab, its bases as the graph spells them."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._gaf_text(gaf, lambda t, k: _check(_lib.lib().flatgfa_gaf_seqs(self._h, t, k, ctypes.byref(p), ctypes.byref(n)), "gaf_seqs"))
        return _take_text(p, n)

    def gaf_table(self, gaf) -> bytes:
        """The bytes `fgfa gaf GAF` prints: per read its name, then which stretch of each segment it covers."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._gaf_text(gaf, lambda t, k: _check(_lib.lib().flatgfa_gaf_table(self._h, t, k, ctypes.byref(p), ctypes.byref(n)), "gaf_table"))
        return _take_text(p, n)

    def all_reads(self, gaf):
        """flatgfa-py's FlatGFA.all_reads (flatgfa.pyi:87): the reads of a GAF file (a name, or bytes) as GAFLines, each an
        iterable of ChunkEvents -- views over the arrays of one device lookup."""
        from . import gaf as _gaf
        _v, pools = self._views()

        def call(ptr, n):
            text = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)) if n else np.zeros(0, np.uint8)
            return _gaf.all_reads(self, pools, self._h, text)
        return self._gaf_text(gaf, call)

    def print_gaf_lookup(self, gaf) -> None:
        """flatgfa-py's FlatGFA.print_gaf_lookup (flatgfa.pyi:88): the `-s` text, to stdout."""
        import sys
        out = self.gaf_seqs(gaf)
        sys.stdout.flush()
        if hasattr(sys.stdout, "buffer"):
            sys.stdout.buffer.write(out)
        else:  # (a text-only stand-in for stdout)
            sys.stdout.write(out.decode(errors="replace"))
        sys.stdout.flush()

    # ---- chop (ops/chop.rs) ----
    def chop(self, max_size: int, links: bool = False) -> "FlatGFA":
        """`fgfa chop -c max_size [-l]`: a new graph whose segments are at most max_size long (flatgfa/src/ops/chop.rs),
        computed on the GPU.  The result owns its pools and outlives this graph."""
        h = ctypes.c_void_p()
        _check(_lib.lib().flatgfa_chop(self._h, int(max_size), 1 if links else 0, ctypes.byref(h)), "chop")
        return FlatGFA(h.value)

    # ---- crush (slow_odgi/crush.py) ----
    def crush(self) -> "FlatGFA":
        """`fgfa crush`: a new graph in which every run of N inside a segment's sequence is a single N (slow_odgi/crush.py,
        `odgi crush`), computed on the GPU.  Segments lose their optional fields and paths their overlaps; the sequence pool
        is laid out again in segment order.  The result owns its pools and outlives this graph."""
        h = ctypes.c_void_p()
        _check(_lib.lib().flatgfa_crush(self._h, ctypes.byref(h)), "crush")
        return FlatGFA(h.value)

    # ---- flip (slow_odgi/flip.py) ----
    def flip(self) -> "FlatGFA":
        """`fgfa flip`: a new graph in which every path that walks more bases backward than forward is turned around --
        its steps reversed, every orientation toggled, `_inv` appended to its name -- and the links the turned paths need
        are added (overlap 0M) and all links de-duplicated, a link and its reverse complement being one (slow_odgi/flip.py,
        `odgi flip`), computed on the GPU.  Paths lose their overlaps and segments their optional fields; the steps are laid
        out again in path order.  The result owns its pools and outlives this graph."""
        h = ctypes.c_void_p()
        _check(_lib.lib().flatgfa_flip(self._h, ctypes.byref(h)), "flip")
        return FlatGFA(h.value)

    def flip_count(self) -> Tuple[int, int]:
        """What :meth:`flip` would do, counted on the GPU without building the graph: (paths that turn, links of the
        result)."""
        turned, links = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.lib().flatgfa_flip_count(self._h, ctypes.byref(turned), ctypes.byref(links)), "flip_count")
        return int(turned.value), int(links.value)

    # ---- inject (slow_odgi/inject.py) ----
    def inject(self, bed, links: bool = False) -> "FlatGFA":
        """`fgfa inject -b BED [-l]`: a new graph in which every BED line "path start end new_name" is a path of its own:
        the segments under the interval's two ends are cut so that both fall on seams, and the new path walks exactly the
        interval (slow_odgi/inject.py, `odgi inject`), computed on the GPU.  `bed` is the BED text (bytes or str) or a list
        of (path, start, end, new_name) with path a name or a path id.  A line of BED text whose path the graph lacks is
        skipped; in a list it is a KeyError.  The result owns its pools and outlives this graph."""
        h = ctypes.c_void_p()
        L = _lib.lib()
        if isinstance(bed, str):
            bed = bed.encode()
        if isinstance(bed, (bytes, bytearray, memoryview)):
            text = bytes(bed)
            _check(L.flatgfa_inject_bed(self._h, text, len(text), 1 if links else 0, ctypes.byref(h)), "inject")
            return FlatGFA(h.value)
        lines = list(bed)
        n = len(lines)
        ids = np.empty(n, np.uint32)
        lo = np.empty(n, np.uint64)
        hi = np.empty(n, np.uint64)
        names = []
        for k, (path, start, end, new) in enumerate(lines):
            if isinstance(path, (int, np.integer)):
                ids[k] = int(path)
            else:
                raw = path.encode() if isinstance(path, str) else bytes(path)
                p = L.flatgfa_find_path(self._h, raw, len(raw))
                if p < 0:
                    raise KeyError(f"path not found: {path!r}")
                ids[k] = p
            lo[k], hi[k] = int(start), int(end)
            names.append(new.encode() if isinstance(new, str) else bytes(new))
        c_names = (ctypes.c_char_p * max(n, 1))(*names)
        c_lens = (ctypes.c_size_t * max(n, 1))(*[len(x) for x in names])
        _check(L.flatgfa_inject(self._h, ids.ctypes.data, lo.ctypes.data, hi.ctypes.data, c_names, c_lens, n, 1 if links else 0,
                                ctypes.byref(h)), "inject")
        return FlatGFA(h.value)

    # ---- extract (ops/extract.rs) and position (ops/position.rs) ----
    def find_seg(self, name: int) -> Optional[int]:
        """The id of the first segment called `name` (FlatGFA::find_seg), or None."""
        i = _lib.lib().flatgfa_find_seg(self._h, int(name))
        return None if i < 0 else int(i)

    def extract(self, seg_name: int, link_distance: int, max_distance_subpaths: int = 300000, num_iterations: int = 6) -> "FlatGFA":
        """`fgfa extract -n seg_name -c link_distance [-d max_distance_subpaths] [-e num_iterations]`: the subgraph within
        link_distance links of the segment, with the subpaths through it (flatgfa/src/ops/extract.rs), computed on the GPU.
        KeyError when no segment has that name.  The result owns its pools and outlives this graph."""
        origin = self.find_seg(seg_name)
        if origin is None:
            raise KeyError("segment not found")
        h = ctypes.c_void_p()
        _check(_lib.lib().flatgfa_extract(self._h, origin, int(link_distance), int(max_distance_subpaths), int(num_iterations),
                                          ctypes.byref(h)), "extract")
        return FlatGFA(h.value)

    def position(self, path_name: bytes, offset: int) -> Optional[Tuple[int, int, bool]]:
        """`fgfa position -p path_name,offset,+`: (segment name, offset into the step, forward?) of the step of the path that
        holds base `offset`, or None past the path's end (flatgfa/src/ops/position.rs).  KeyError for an unknown path."""
        p = self.find_path(path_name)
        if p is None:
            raise KeyError("path not found")
        hd, off, found = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_int()
        _check(_lib.lib().flatgfa_position(self._h, p, int(offset), ctypes.byref(hd), ctypes.byref(off), ctypes.byref(found)), "position")
        if not found.value:
            return None
        return int(self.pool("segs")["name"][hd.value >> 1]), int(off.value), (hd.value & 1) == 0

    def position_table(self, triple: bytes) -> bytes:
        """The bytes `fgfa position -p triple` prints."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_position_table(self._h, triple, len(triple), ctypes.byref(p), ctypes.byref(n)), "position")
        return _take_text(p, n)

    # ---- validate (slow_odgi/validate.py) and degree (slow_odgi/degree.py) ----
    def validate(self) -> np.ndarray:
        """`fgfa validate` as records: one per pair of consecutive steps of a path that no link supports, in path order then
        step order (slow_odgi/validate.py:9-24) -- `path`, `step` (the index of the pair's first step in its path), and the
        two handles `src` and `dst` (segment << 1 | backward).  Empty for a graph whose paths are walks of it."""
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        _check(_lib.lib().flatgfa_validate(self._h, ctypes.byref(out), ctypes.byref(n)), "validate")
        try:
            if not n.value:
                return np.zeros(0, MISSING_LINK_DT)
            raw = (ctypes.c_char * (n.value * MISSING_LINK_DT.itemsize)).from_address(out.value)  # (string_at takes a C int)
            return np.frombuffer(raw, MISSING_LINK_DT).copy()
        finally:
            _lib.lib().flatgfa_missing_links_free(out)

    def validate_count(self) -> int:
        """How many records validate() would return, without fetching them."""
        n = ctypes.c_uint64()
        _check(_lib.lib().flatgfa_validate(self._h, None, ctypes.byref(n)), "validate")
        return int(n.value)

    def validate_table(self) -> bytes:
        """The bytes `fgfa validate` prints: nothing for a valid graph."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_validate_table(self._h, ctypes.byref(p), ctypes.byref(n)), "validate")
        return _take_text(p, n)

    def degree(self) -> np.ndarray:
        """slow_odgi/degree.py:9-17 -> link ends per segment, uint64, indexed by segment id."""
        d = np.zeros(max(self.segment_count, 1), np.uint64)
        _check(_lib.lib().flatgfa_degree(self._h, d.ctypes.data), "degree")
        return d[:self.segment_count]

    def degree_table(self) -> bytes:
        """The bytes `fgfa degree` prints."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_degree_table(self._h, ctypes.byref(p), ctypes.byref(n)), "degree")
        return _take_text(p, n)

    # ---- flatten (slow_odgi/flatten.py) ----
    def flatten_legend(self) -> np.ndarray:
        """slow_odgi/flatten.py:13-19 -> uint64[segment_count + 1]: the bases before each segment in pool order, then all of
        them; segment s lies at [legend[s], legend[s + 1]) of the FASTA's bases."""
        out = np.zeros(self.segment_count + 1, np.uint64)
        _check(_lib.lib().flatgfa_flatten_legend(self._h, out.ctypes.data), "flatten_legend")
        return out

    def flatten_fasta(self, name: bytes) -> bytes:
        """The FASTA record `slow_odgi flatten` prints (flatten.py:51-55): `>name`, then every segment's bases, 80 to a line."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_flatten_fasta(self._h, name, len(name), ctypes.byref(p), ctypes.byref(n)), "flatten_fasta")
        return _take_text(p, n)

    def flatten_bed(self, name: bytes) -> bytes:
        """The BED table `slow_odgi flatten` prints (flatten.py:23-41): per path step where its segment lies in the FASTA."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib.lib().flatgfa_flatten_bed(self._h, name, len(name), ctypes.byref(p), ctypes.byref(n)), "flatten_bed")
        return _take_text(p, n)

    def flatten_stream(self, name: bytes, what: int, write) -> None:
        """flatgfa_flatten_stream: `write(bytes)` receives the text in order, a piece at a time (what: 1 the FASTA, 2 the BED,
        3 both, the FASTA first).  A `write` that raises, or returns something true, stops the call."""
        raised = []

        def sink(_ctx, ptr, n):
            try:
                return 1 if write(ctypes.string_at(ptr, n)) else 0  # (a piece is a few megabytes: within string_at's C int)
            except BaseException as e:  # noqa: BLE001  (must not unwind through the C caller)
                raised.append(e)
                return 1
        rc = _lib.lib().flatgfa_flatten_stream(self._h, name, len(name), int(what), _lib.SINK_T(sink), None)
        if raised:
            raise raised[0]
        _check(rc, "flatten_stream")

    def flatten_to(self, name: bytes, fasta_file=None, bed_file=None) -> None:
        """`odgi flatten -f FASTA -b BED`: the FASTA and the BED into open binary files, written as they stream from the
        device (either may be None)."""
        for f, what in ((fasta_file, 1), (bed_file, 2)):
            if f is not None:
                self.flatten_stream(name, what, lambda b, f=f: f.write(b) and None)


MISSING_LINK_DT =np.dtype([("path", "<u4"), ("step", "<u4"), ("src", "<u4"), ("dst", "<u4")])  # flatgfa_missing_link_t

SHARD_WHOLE_PATHS = 1  # FLATGFA_SHARD_WHOLE_PATHS
SHARD_NO_RCCL = 2      # FLATGFA_SHARD_NO_RCCL


class ShardedFlatGFA:
    """One graph sharded over the GPUs of a node by this process (`flatgfa_sharded_t`): the local
    kernels on every shard, one RCCL all-reduce of the fused [depth | uniq] vector, results as the
    single-device calls give them.  `devices[i]` is shard i's HIP device (default: shard i on
    device i mod the device count); devices may repeat (shards that share one exchange by
    device-side adds)."""

    def __init__(self, graph: FlatGFA, n_shards: int, devices: Optional[Sequence[int]] = None, flags: int = 0):
        self.graph = graph  # the handle borrows the graph
        self.n_shards = int(n_shards)
        arr = None
        if devices is not None:
            if len(devices) != self.n_shards:
                raise ValueError("one device per shard")
            arr = (ctypes.c_int * self.n_shards)(*[int(d) for d in devices])
        self._h = ctypes.c_void_p(_lib.lib().flatgfa_sharded_create(graph._h, arr, self.n_shards, int(flags)))
        if not self._h.value:
            raise FlatGFAError(f"flatgfa_sharded_create: {_lib.last_error()}")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().flatgfa_sharded_free(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "ShardedFlatGFA":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def layout(self) -> List[dict]:
        """Per shard: its device, its stretch of the steps pool, the first path it walks, how many
        paths or pieces it walks; plus how many paths the handle cuts and whether RCCL carries the exchange."""
        out = []
        for i in range(self.n_shards):
            dev, uses = ctypes.c_int(), ctypes.c_int()
            b, e = ctypes.c_uint64(), ctypes.c_uint64()
            fp, npc, nsp = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
            _check(_lib.lib().flatgfa_sharded_layout(self._h, i, ctypes.byref(dev), ctypes.byref(b), ctypes.byref(e), ctypes.byref(fp),
                                                     ctypes.byref(npc), ctypes.byref(nsp), ctypes.byref(uses)), "sharded_layout")
            out.append({"device": dev.value, "step_begin": b.value, "step_end": e.value, "first_path": fp.value,
                        "pieces": npc.value, "split_paths": nsp.value, "rccl": bool(uses.value)})
        return out

    def collective_bytes(self, with_uniq: bool = True) -> int:
        """Bytes every shard contributes to the one collective of a call (the cut paths' touch counters travel packed)."""
        return int(_lib.lib().flatgfa_sharded_collective_bytes(self._h, 1 if with_uniq else 0))

    def seg_depth_with_uniq(self) -> Tuple[np.ndarray, np.ndarray]:
        S = self.graph.segment_count
        d, u = np.zeros(S, dtype=np.uint64), np.zeros(S, dtype=np.uint64)
        _check(_lib.lib().flatgfa_sharded_seg_depth(self._h, d.ctypes.data, u.ctypes.data), "sharded_seg_depth")
        return d, u

    def seg_depth(self) -> np.ndarray:
        d = np.zeros(self.graph.segment_count, dtype=np.uint64)
        _check(_lib.lib().flatgfa_sharded_seg_depth(self._h, d.ctypes.data, None), "sharded_seg_depth")
        return d

    def path_depth(self, path_ids: Optional[Iterable[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        ids = np.arange(self.graph.path_count, dtype=np.uint32) if path_ids is None else np.asarray(list(path_ids), dtype=np.uint32)
        ln, mean = np.zeros(len(ids), dtype=np.uint64), np.zeros(len(ids), dtype=np.float64)
        _check(_lib.lib().flatgfa_sharded_path_depth(self._h, ids.ctypes.data if len(ids) else None, len(ids),
                                                     ln.ctypes.data if len(ids) else None, mean.ctypes.data if len(ids) else None),
               "sharded_path_depth")
        return ln, mean

    def ranks_seen(self) -> int:
        """How many ranks the handle's exchange really spans (an all-reduce of ones over its communicator)."""
        n = int(_lib.lib().flatgfa_sharded_ranks_seen(self._h))
        if n < 0:
            _check(n, "sharded_ranks_seen")
        return n

    def enqueue(self, with_uniq: bool = True) -> None:
        _check(_lib.lib().flatgfa_sharded_enqueue(self._h, 1 if with_uniq else 0), "sharded_enqueue")

    def sync(self) -> None:
        _check(_lib.lib().flatgfa_sharded_sync(self._h), "sharded_sync")

    def fetch(self, shard: int = 0, with_uniq: bool = True):
        S = self.graph.segment_count
        d = np.zeros(S, dtype=np.uint64)
        u = np.zeros(S, dtype=np.uint64) if with_uniq else None
        _check(_lib.lib().flatgfa_sharded_fetch(self._h, int(shard), d.ctypes.data, u.ctypes.data if with_uniq else None), "sharded_fetch")
        return (d, u) if with_uniq else d


def shard_cuts(path_steps, n_shards: int, flags: int = 0) -> np.ndarray:
    """Where `ShardedFlatGFA` cuts a graph whose paths, in path order, have `path_steps[p]` steps
    (flatgfa_shard_cuts: host only, no device needed): n_shards + 1 cut points counted in path steps along
    the path order; shard r walks [cuts[r], cuts[r + 1])."""
    ps = np.ascontiguousarray(path_steps, dtype=np.uint64)
    out = np.zeros(int(n_shards) + 1, dtype=np.uint64)
    _check(_lib.lib().flatgfa_shard_cuts(ps.ctypes.data if len(ps) else None, len(ps), int(n_shards), int(flags), out.ctypes.data), "shard_cuts")
    return out


def parse(filename: Union[str, os.PathLike]) -> FlatGFA:
    """Parse a GFA text file (flatgfa_parse, flatgfa-c/src/lib.rs:63)."""
    return FlatGFA(_lib.lib().flatgfa_parse(os.fsencode(filename)))


def parse_bytes(gfa: bytes) -> FlatGFA:
    return FlatGFA(_lib.lib().flatgfa_parse_bytes(gfa, len(gfa)))


def parse_stream_bytes(gfa: bytes) -> FlatGFA:
    return FlatGFA(_lib.lib().flatgfa_parse_stream_bytes(gfa, len(gfa)))


PARSE_REASONS = ("plain", "grammar", "name", "limit")


def parse_device_info() -> dict:
    """This thread's last device-parse call (flatgfa_parse_device_info, flatgfa_parse_device_times): the route taken ("device" or
    "host"), why, the step kernels' text tile in bytes, the tiles of the text, and the call's milliseconds."""
    info = (ctypes.c_uint64 * 4)()
    ms = (ctypes.c_double * 4)()
    _check(_lib.lib().flatgfa_parse_device_info(info), "parse_device_info")
    _check(_lib.lib().flatgfa_parse_device_times(ms), "parse_device_times")
    return {"parsed_on": "device" if info[0] else "host", "reason": PARSE_REASONS[info[1]], "tile_bytes": int(info[2]), "tiles": int(info[3]),
            "upload_ms": ms[0], "kernel_ms": ms[1], "step_ms": ms[2], "download_ms": ms[3]}


def _parsed_on_device(handle: int) -> FlatGFA:
    g = FlatGFA(handle)
    info = parse_device_info()
    g.parsed_on, g.parse_reason, g.parse_info = info["parsed_on"], info["reason"], info
    return g


def parse_bytes_device(gfa: bytes, stream: bool = False) -> FlatGFA:
    """The graph of parse_bytes (stream=False) or parse_stream_bytes (stream=True), its pools made on the GPU where the text is
    of the plain grammar and by the host parser where it is not: `parsed_on` says which ("device" or
    "host"), `parse_reason` why ("plain", "grammar", "name", "limit").  Without a device: FlatGFAError."""
    return _parsed_on_device(_lib.lib().flatgfa_parse_bytes_device(gfa, len(gfa), 1 if stream else 0))


def parse_device(filename) -> FlatGFA:
    """parse(filename) through the device route (flatgfa_parse_device)."""
    return _parsed_on_device(_lib.lib().flatgfa_parse_device(os.fsencode(filename)))


def translate_prealloc(gfa: bytes, filename: Union[str, os.PathLike], factor: int = 32, from_stream: bool = False) -> None:
    """`fgfa -m -p FACTOR -o OUT [-I GFA]` (cli/main.rs:216-248): the text is parsed straight into the
    mapped, preallocated output file (file.rs:255-272); no graph is built in between.  `from_stream`:
    the text came from stdin (capacities guessed from `factor`, parse_stream's rules)."""
    _check(_lib.lib().flatgfa_translate_prealloc(gfa, len(gfa), 1 if from_stream else 0, os.fsencode(filename), int(factor)),
           "translate_prealloc")


def load(filename: Union[str, os.PathLike]) -> FlatGFA:
    """Map a binary `.flatgfa` file (file::view, flatgfa/src/file.rs:185)."""
    return FlatGFA(_lib.lib().flatgfa_load(os.fsencode(filename)))


def synth(seed: int, n_segs: int, n_paths: int, steps_per_path: int, model: str = "pangenome",
          with_seq: bool = False) -> FlatGFA:
    """The deterministic synthetic graph of SURVEY.md 8(d)."""
    m = {"pangenome": 0, "uniform": 1, "chromosome": 2, "haplotype": 3, "repeats": 4}[model]
    return FlatGFA(_lib.lib().flatgfa_synth(seed, n_segs, n_paths, steps_per_path, m, with_seq))


# ---- the packed-sequence codec (flatgfa/src/packedseq.rs; `fgfa seq-export`, `fgfa seq-import`) ----
def seq_export(text: bytes) -> bytes:
    """`fgfa seq-export`: the packed file image of nucleotide text, made on the GPU -- a 25-byte header, then two bases a byte
    (A 0, C 1, T 2, G 3; the even base in the low nibble).  Whitespace is dropped; any other byte that is not one of A C T G
    raises FlatGFAError (code -7) naming the smallest offending offset."""
    text = bytes(text)
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(_lib.lib().flatgfa_seq_export(text, len(text), ctypes.byref(p), ctypes.byref(n)), "seq_export")
    return _take_text(p, n)


def seq_export_file(text: bytes, filename: Union[str, os.PathLike]) -> None:
    """seq_export into a file; on an error no file is made."""
    text = bytes(text)
    _check(_lib.lib().flatgfa_seq_export_file(text, len(text), os.fsencode(filename)), "seq_export_file")


def seq_import(packed: bytes) -> bytes:
    """`fgfa seq-import` without its newline: the bases of a packed file image, unpacked on the GPU.  A malformed header or a
    nibble above 3 raises FlatGFAError (code -7)."""
    packed = bytes(packed)
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(_lib.lib().flatgfa_seq_import(packed, len(packed), ctypes.byref(p), ctypes.byref(n)), "seq_import")
    return _take_text(p, n)


def seq_import_file(filename: Union[str, os.PathLike]) -> bytes:
    """seq_import of a file's contents."""
    with open(filename, "rb") as f:
        return seq_import(f.read())


def seq_packed_info(packed: bytes) -> Tuple[int, int]:
    """(the number of bases, the offset of the data bytes) of a packed file image: the header checks alone, on the host."""
    packed = bytes(packed)
    bases, off = ctypes.c_uint64(), ctypes.c_uint64()
    _check(_lib.lib().flatgfa_seq_packed_info(packed, len(packed), ctypes.byref(bases), ctypes.byref(off)), "seq_packed_info")
    return bases.value, off.value


# ---- BED intersection (flatgfa/src/cli/cmds.rs:392-413; `fgfa bed -a FILE -b FILE`) ----
def _bed_text(x) -> bytes:
    """BED text given as bytes, or as the path of a file that holds it."""
    if isinstance(x, (str, os.PathLike)):
        with open(x, "rb") as f:
            return f.read()
    return bytes(x)


def bed_intersect(a, b) -> bytes:
    """`fgfa bed -a A -b B`: for every entry of `a` in file order, the entries of `b` of the same name that overlap it, in
    file order, cut to the overlap -- "name<TAB>start<TAB>end" lines, byte for byte the reference's -- found and formatted on
    the GPU.  a and b are BED text (bytes) or paths."""
    a, b = _bed_text(a), _bed_text(b)
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(_lib.lib().flatgfa_bed_intersect(a, len(a), b, len(b), ctypes.byref(p), ctypes.byref(n)), "bed_intersect")
    return _take_text(p, n)


def bed_intersect_stream(a, b, write) -> None:
    """flatgfa_bed_intersect_stream: `write(bytes)` receives the text of bed_intersect(a, b) in order, a piece at a time; never
    called where there is no line to print.  A `write` that raises, or returns something true, stops the call."""
    a, b = _bed_text(a), _bed_text(b)
    raised = []

    def sink(_ctx, ptr, n):
        try:
            return 1 if write(ctypes.string_at(ptr, n)) else 0  # (a piece is a few megabytes: within string_at's C int)
        except BaseException as e:  # noqa: BLE001  (must not unwind through the C caller)
            raised.append(e)
            return 1
    rc = _lib.lib().flatgfa_bed_intersect_stream(a, len(a), b, len(b), _lib.SINK_T(sink), None)
    if raised:
        raise raised[0]
    _check(rc, "bed_intersect_stream")


def bed_intersect_count(a, b) -> Tuple[int, int, int, int]:
    """(lines, bytes, candidates, unsorted_groups) of bed_intersect(a, b) without its text: how long the text is, how many
    pairs of entries were tried, and how many of b's name groups were walked whole because their starts are not in order."""
    a, b = _bed_text(a), _bed_text(b)
    out = [ctypes.c_uint64() for _ in range(4)]
    _check(_lib.lib().flatgfa_bed_intersect_count(a, len(a), b, len(b), *[ctypes.byref(x) for x in out]), "bed_intersect_count")
    return tuple(x.value for x in out)


def format_float(x: float, digits: int) -> str:
    buf = ctypes.create_string_buffer(600)
    n = _lib.lib().flatgfa_format_float(x, digits, buf, 600)
    return buf.raw[:n].decode()


def device_count() -> int:
    return _lib.lib().flatgfa_device_count()
