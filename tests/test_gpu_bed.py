"""BED intersection on the GPU against tests/bed_model.py, byte for byte: every shape of tests/bed_shapes.py through the whole
call, the stream, the count, the CLI and the device-level call.  Run with -m gpu."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bed_model as bm
import bed_shapes as bs
import pollen_amd as pa
from conftest import GOLDEN, ROOT
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def check(a: bytes, b: bytes) -> bytes:
    """whole call == stream concatenated == the model; count's lines and bytes are the text's"""
    want = bm.intersect(a, b)
    assert pa.bed_intersect(a, b) == want
    pieces = []
    pa.bed_intersect_stream(a, b, pieces.append)
    assert b"".join(pieces) == want
    if not want:
        assert pieces == []  # (the sink is never called)
    lines, nbytes, cands, _unsorted = pa.bed_intersect_count(a, b)
    assert (lines, nbytes) == (want.count(b"\n"), len(want)) and cands >= lines
    return want


@pytest.mark.parametrize("name", list(bs.SHAPES))
def test_shape(name):
    check(*bs.SHAPES[name])


@pytest.mark.parametrize("name", list(bs.SHAPES))
def test_cli(name, tmp_path):
    a, b = bs.SHAPES[name]
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(a)
    fb.write_bytes(b)
    r = subprocess.run([FGFA, "bed", "-a", str(fa), "-b", str(fb)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    assert r.stdout == bm.intersect(a, b)
    assert pa.bed_intersect(fa, str(fb)) == r.stdout  # (paths)


def test_a_sink_that_stops():
    a = bs.text(bs.run(b"chr1", 300_000, 10, 0, at=1_000_000))
    b = b"chr1\t0\t999999999\n"
    want = bm.intersect(a, b)
    assert len(want) > bs.PIECE  # two pieces would travel
    got = []

    def stop_after_one(p):
        got.append(p)
        return True
    with pytest.raises(pa.FlatGFAError) as e:
        pa.bed_intersect_stream(a, b, stop_after_one)
    assert e.value.code == -5 and "bed: " in _lib.last_error()  # FLATGFA_ERR_IO
    assert len(got) == 1 and want.startswith(got[0]) and 0 < len(got[0]) < len(want)

    class Stop(Exception):
        pass

    def raises(p):
        raise Stop()
    with pytest.raises(Stop):
        pa.bed_intersect_stream(a, b, raises)
    assert pa.bed_intersect(a, b) == want  # (the next call answers as before)


def test_zero_hits():
    a, b = bs.SHAPES["no hit"]
    called = []
    pa.bed_intersect_stream(a, b, called.append)
    assert called == [] and pa.bed_intersect(a, b) == b""
    assert pa.bed_intersect_count(a, b)[:2] == (0, 0)
    text, n = ctypes.c_void_p(), ctypes.c_size_t(7)
    assert _lib.lib().flatgfa_bed_intersect(a, len(a), b, len(b), ctypes.byref(text), ctypes.byref(n)) == 0
    assert n.value == 0 and ctypes.string_at(text.value, 1) == b"\0"  # (NUL-terminated)
    _lib.lib().flatgfa_free_text(text)


@pytest.mark.parametrize("graph", ["ref_ex1", "kat_window_depth"])
def test_flatten_bed_against_an_annotation(graph):
    """-a is what `fgfa flatten -b` writes: six columns under a `#` header, in linear coordinates."""
    name = graph.encode() + b".og"
    with pa.parse(os.path.join(GOLDEN, graph + ".gfa")) as g:
        a = g.flatten_bed(name)
    assert a.startswith(b"#name\tstart\tend\t") and a.count(b"\n") > 3
    total = max(e for _, _, e in bm.parse(a))
    b = b"%s\t0\t%d\tfirst\n%s\t%d\t%d\tsecond\nelsewhere\t0\t%d\tthird\n" % (name, total // 2, name, total // 3, total, total)
    want = check(a, b)
    assert want.count(b"\n") >= a.count(b"\n") - 1  # every step lies under the first or the second


def tensors(entries, ids, order=None):
    import torch
    order = range(len(entries)) if order is None else order
    rows = [entries[k] for k in order]
    dev = torch.device("cuda", 0)

    def u64(vals):
        return torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(dev)
    return (torch.tensor([ids.get(r[0], -1) for r in rows], dtype=torch.int32, device=dev), u64([r[1] for r in rows]), u64([r[2] for r in rows]))


def device_records(a: bytes, b: bytes, **kw):
    """(got, want): the device-level call's records and the model's pairs, b's index in grouped order"""
    from pollen_amd import device
    ea, eb = bm.parse(a), bm.parse(b)
    ids, order = bm.grouped(eb)
    at = {k: j for j, k in enumerate(order)}
    want = [(i, at[k], s, e) for i, k, s, e in bm.pairs(ea, eb)]
    out = device.bed_intersect(*tensors(ea, ids), *tensors(eb, ids, order), n_groups=len(ids), **kw)
    ai, bi, s, e = (t.cpu().numpy() for t in out)
    got = list(zip(ai.tolist(), bi.tolist(), s.view(np.uint64).tolist(), e.view(np.uint64).tolist()))
    return got, want


@pytest.mark.parametrize("name", list(bs.SHAPES))
def test_device_level_records(name):
    got, want = device_records(*bs.SHAPES[name])
    assert got == want


def test_device_level_refusals():
    import torch
    from pollen_amd import device
    dev = torch.device("cuda", 0)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    def i64(v):
        return torch.tensor(v, dtype=torch.int64, device=dev)
    a = (i32([0]), i64([0]), i64([9]))
    for b_ids, n_groups in [([1, 0], 2), ([0, 2], 2), ([0, 1], 1)]:  # not grouped; an id at or past the group count
        with pytest.raises(pa.FlatGFAError) as e:
            device.bed_intersect(*a, i32(b_ids), i64([0, 1]), i64([5, 6]), n_groups=n_groups)
        assert e.value.code == -2 and "bed: " in _lib.last_error()
    with pytest.raises(pa.FlatGFAError) as e:
        device.bed_intersect(i32([3]), i64([0]), i64([9]), i32([0, 1]), i64([0, 1]), i64([5, 6]), n_groups=2)
    assert e.value.code == -2
    out = device.bed_intersect(i32([-1, 1]), i64([0, 0]), i64([9, 9]), i32([0, 1]), i64([0, 1]), i64([5, 6]), n_groups=2)
    assert [t.tolist() for t in out] == [[1], [1], [1], [6]]
