"""What flatten says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only route says
("no HIP device is visible; <route> has no CPU fallback", tests/test_no_device_messages.py).  Skipped where a device is
visible.  Argument errors are answered without a device, there and here."""
import ctypes
import io

import pytest

import pollen_amd as pa
from pollen_amd import _lib

TEXT = b"S\t1\tACGT\nS\t2\tAC\nS\t3\tG\nP\tp\t1+,2+,3-\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t-\t0M\n"
MESSAGE = "no HIP device is visible; flatten has no CPU fallback"

ROUTES = {
    "legend": lambda g: g.flatten_legend(),
    "fasta": lambda g: g.flatten_fasta(b"x.og"),
    "bed": lambda g: g.flatten_bed(b"x.og"),
    "to files": lambda g: g.flatten_to(b"x.og", io.BytesIO(), io.BytesIO()),
    "stream": lambda g: g.flatten_stream(b"x.og", 3, lambda b: None),
}


@pytest.mark.parametrize("what", list(ROUTES))
def test_no_device_message(what):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            ROUTES[what](g)
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == MESSAGE
    finally:
        g.close()


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    g = pa.parse_bytes(TEXT)
    sink = _lib.SINK_T(lambda ctx, p, n: 0)
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    try:
        assert lib.flatgfa_flatten_stream(g._h, b"x", 1, 0, sink, None) == -1  # `what` outside 1..3
        assert lib.flatgfa_flatten_stream(g._h, b"x", 1, 4, sink, None) == -1
        assert lib.flatgfa_flatten_stream(g._h, b"x", 1, 3, None, None) == -1  # no sink
        assert lib.flatgfa_flatten_stream(g._h, None, 1, 3, sink, None) == -1  # a length and no name
        assert lib.flatgfa_flatten_stream(None, b"x", 1, 3, sink, None) == -1
        assert lib.flatgfa_flatten_fasta(g._h, None, 2, ctypes.byref(p), ctypes.byref(n)) == -1
        assert lib.flatgfa_flatten_bed(g._h, b"x", 1, None, ctypes.byref(n)) == -1
        assert lib.flatgfa_flatten_legend(g._h, None) == -1
        assert lib.flatgfa_dev_flatten_legend(None, None, None) == -1
        graph = _lib.flatgfa_dev_graph_t()  # (no seg_len)
        assert lib.flatgfa_dev_flatten_legend(ctypes.byref(graph), ctypes.c_void_p(16), None) == -1
        assert "seg_len" in _lib.last_error()
    finally:
        g.close()
