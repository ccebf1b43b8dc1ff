"""crush at its kernels' seams (tests/crush_shapes.py: tile edges, empty segments, output vectors, scan tiles, aliased spans),
its refusals, laid-out offsets past 2^32 and a stream of the caller's.  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import crush_gpu as cg
import crush_model as cm
import crush_shapes as cs
import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
T = cs.T


@pytest.mark.parametrize("name", list(cs.SHAPES))
def test_shape_device_pair(name):
    p = cs.SHAPES[name]()
    cg.check_device_pair(p, cm.crush_fast(p), what=name)


HANDLE_SHAPES = [n for n in cs.SHAPES if n not in ("more tiles than workgroups",)]


@pytest.mark.parametrize("name", HANDLE_SHAPES)
def test_shape_handle(name, tmp_path):
    p = cs.SHAPES[name]()
    path = tmp_path / "g.flatgfa"
    path.write_bytes(fo.dump_flatgfa(p))
    g = pa.load(str(path))
    q = g.crush()
    cm.assert_same_pools(cm.pools_of(q), cm.crush_fast(p), name)
    q.close()
    g.close()


def test_empty_segments_start_where_the_next_segment_begins():
    # the rule for a segment without a first byte: it starts at the sum of the new lengths before it
    p = cs.SHAPES["empty segments at a tile edge"]()
    _, _, spans = cg.check_device_pair(p, cm.crush_fast(p))
    s = cg.u32(spans)
    assert s[2::2][:3].tolist() == [T, T, T] and s[3::2][:3].tolist() == [0, 0, 0]  # three empty ones behind T kept bytes
    assert s[8] == T and s[9] == 2 and s[10] == T + 2 and s[-2] == 2 * T + 2 and s[-1] == 0
    p = cs.SHAPES["only empty segments"]()
    _, seq_out, spans = cg.check_device_pair(p, cm.crush_fast(p))
    assert seq_out.numel() == 0 and not cg.u32(spans).any()


def raw_count(seg_seq, seq, n_segs, seg_len, stream=None):
    job, kept, dropped = ctypes.c_void_p(), ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = _lib.lib().flatgfa_dev_crush_count(seg_seq.data_ptr() if n_segs else None, seq.data_ptr() if seq.numel() else None, seq.numel(), n_segs,
                                            seg_len.data_ptr() if n_segs else None, stream, ctypes.byref(job), ctypes.byref(kept), ctypes.byref(dropped))
    return rc, job, kept.value, dropped.value


def test_a_span_one_past_the_pool_is_refused_and_nothing_is_written():
    import torch
    d = torch.device("cuda:0")
    pool = np.frombuffer(b"ANNNC" * 20, np.uint8)
    seq = torch.from_numpy(pool.copy()).to(d)
    for spans, rc_want in (([0, 50, 50, 50], 0), ([0, 50, 50, 51], -2), ([0, 50, 101, 0], -2), ([0xFFFFFFFF, 2, 0, 1], -2)):
        seg_seq = torch.from_numpy(np.array(spans, np.uint32).view(np.int32)).to(d)
        seg_len = torch.full((2,), -1, dtype=torch.int32, device=d)
        rc, job, kept, dropped = raw_count(seg_seq, seq, 2, seg_len)
        assert rc == rc_want, spans
        if rc:
            assert job.value is None and seg_len.cpu().numpy().tolist() == [-1, -1]
            assert "span outside seq_data" in _lib.last_error()
        else:  # a span that ends exactly at seq_len
            assert (kept, dropped) == (60, 40) and job.value
            _lib.lib().flatgfa_dev_crush_free(job)
            assert seg_len.cpu().numpy().tolist() == [30, 30]


@pytest.mark.parametrize("off", [1, 15])
def test_a_destination_off_16_byte_alignment(off):
    import torch
    d = torch.device("cuda:0")
    p = cs.SHAPES["first drop at T"]()
    want = cm.crush_fast(p)
    _, seg_seq, seq = cg.to_device(p)
    seg_len = torch.zeros(1, dtype=torch.int32, device=d)
    rc, job, kept, dropped = raw_count(seg_seq, seq, 1, seg_len)
    assert rc == 0 and kept == len(want.seq_data) and dropped == 5
    room = torch.full((kept + 64,), 0x55, dtype=torch.uint8, device=d)
    assert room.data_ptr() % 16 == 0
    spans = torch.zeros(2, dtype=torch.int32, device=d)
    try:
        assert _lib.lib().flatgfa_dev_crush_fill(job, room.data_ptr() + 16 + off, spans.data_ptr(), None) == 0
    finally:
        _lib.lib().flatgfa_dev_crush_free(job)
    got = room.cpu().numpy()
    assert got[16 + off:16 + off + kept].tobytes() == want.seq_data.tobytes()
    assert (got[:16 + off] == 0x55).all() and (got[16 + off + kept:] == 0x55).all()  # not a byte beside it
    assert cg.u32(spans).tolist() == [0, kept]


def test_a_stream_of_the_callers():
    import torch
    st = torch.cuda.Stream()
    p = cs.SHAPES["empty segments at a tile edge"]()
    cg.check_device_pair(p, cm.crush_fast(p), stream=st)
    p = cs.SHAPES["out of order, overlapping, aliased"]()
    cg.check_device_pair(p, cm.crush_fast(p), stream=st)


# ---- laid-out offsets past 2^32 (device-level only: no handle holds such a graph's output... or input) ----
POOL = 1 << 28
PLANTED = {0: b"A", 5: b"C", (1 << 27) + 3: b"G", POOL - 1: b"T"}  # the rest is N


def big_spans():
    # seventeen segments that alias all of the pool: 17 * 2^28 laid-out bytes
    return np.array([0, POOL] * 17, np.uint32)


def test_offsets_past_2_to_the_32():
    import torch
    d = torch.device("cuda:0")
    seq = torch.full((POOL,), cm.N, dtype=torch.uint8, device=d)
    for at, ch in PLANTED.items():
        seq[at] = ch[0]
    seg_seq = torch.from_numpy(big_spans().view(np.int32)).to(d)
    seg_len = torch.zeros(17, dtype=torch.int32, device=d)
    rc, job, kept, dropped = raw_count(seg_seq, seq, 17, seg_len)
    # by hand: A N(1..4) C N(6..2^27+2) G N(..2^28-2) T  ->  A N C N G N T, seven bytes a segment
    one = b"ANCNGNT"
    assert rc == 0 and kept == 17 * len(one) and dropped == 17 * (POOL - len(one))
    out = torch.zeros(kept, dtype=torch.uint8, device=d)
    spans = torch.zeros(34, dtype=torch.int32, device=d)
    try:
        assert _lib.lib().flatgfa_dev_crush_fill(job, out.data_ptr(), spans.data_ptr(), None) == 0
    finally:
        _lib.lib().flatgfa_dev_crush_free(job)
    assert out.cpu().numpy().tobytes() == one * 17
    assert seg_len.cpu().numpy().tolist() == [7] * 17
    assert cg.u32(spans).tolist() == [x for s in range(17) for x in (7 * s, 7)]


def test_more_kept_bytes_than_a_span_holds():
    import torch
    d = torch.device("cuda:0")
    seq = torch.full((POOL,), ord("A"), dtype=torch.uint8, device=d)
    seg_seq = torch.from_numpy(big_spans().view(np.int32)).to(d)
    seg_len = torch.full((17,), -1, dtype=torch.int32, device=d)
    rc, job, kept, dropped = raw_count(seg_seq, seq, 17, seg_len)
    assert rc == -6 and job.value is None  # FLATGFA_ERR_TOO_LARGE, no job
    assert str(17 * POOL) in _lib.last_error()
    assert seg_len.cpu().numpy().tolist() == [-1] * 17  # nothing written
    # sixteen of them, less one byte: 2^32 - 1 kept bytes fit
    spans = big_spans()[:32].copy()
    spans[31] = POOL - 1
    seg_seq = torch.from_numpy(spans.view(np.int32)).to(d)
    rc, job, kept, dropped = raw_count(seg_seq, seq, 16, seg_len)
    assert rc == 0 and kept == (1 << 32) - 1 and dropped == 0
    _lib.lib().flatgfa_dev_crush_free(job)
