"""What crush says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only route says.
Skipped where a device is visible.  A span that leaves seq_data and the argument errors are decided before any device work, so
they are answered the same with and without a device, and are tested here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import crush_model as cm
import crush_shapes as cs
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

TEXT = b"S\t1\tANNA\nS\t2\tNN\nS\t3\tGGG\nP\tp\t1+,2-,3+\t*\nL\t1\t+\t2\t-\t0M\n"
MESSAGE = "no HIP device is visible; crush has no CPU fallback"
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def test_no_device_message():
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            g.crush()
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == MESSAGE
    finally:
        g.close()


@pytest.mark.parametrize("how", ["text", "-o"])
def test_cli_without_a_device(tmp_path, how):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    gfa, out = tmp_path / "g.gfa", tmp_path / "o.flatgfa"
    gfa.write_bytes(TEXT)
    args = [FGFA, "-I", str(gfa)] + (["-o", str(out)] if how == "-o" else []) + ["crush"]
    r = subprocess.run(args, capture_output=True, timeout=120)
    assert r.returncode == 1 and MESSAGE.encode() in r.stderr and r.stdout == b"" and not out.exists()


def poke_span(g, seg, start, end):
    """Segment `seg` of a heap handle gets the sequence span (start, end), behind the library's back: the loaders refuse a
    file with such a span, so this is the one way a handle comes to hold it."""
    data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, fo.POOL_ORDER.index("segs"), ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
    assert es.value == 24 and seg < n.value
    words = ctypes.cast(data.value + 24 * seg + 8, ctypes.POINTER(ctypes.c_uint32))
    words[0], words[1] = start, end


@pytest.mark.parametrize("span", [(2, 10), (3, 2), (20, 20)], ids=["one past the pool", "start after end", "empty, past the pool"])
def test_a_bad_span_is_refused_before_any_device_work(span):
    # (with or without a device: BOUNDS, never NO_DEVICE -- the spans are checked first)
    g = pa.parse_bytes(TEXT)  # (9 bytes of seq_data)
    try:
        assert len(g.pool("seq_data")) == 9
        poke_span(g, 1, *span)
        with pytest.raises(pa.FlatGFAError) as e:
            g.crush()
        assert e.value.code == -2  # FLATGFA_ERR_BOUNDS
        assert _lib.last_error() == "crush: segment 1 has a sequence span outside seq_data"
        poke_span(g, 1, 4, 9)  # a span that ends exactly at the pool's end is not refused for that: the next answer is the device's
        if pa.device_count() == 0:
            with pytest.raises(pa.FlatGFAError) as e:
                g.crush()
            assert e.value.code == -3
    finally:
        g.close()


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    g = pa.parse_bytes(TEXT)
    out = ctypes.c_void_p()
    n = ctypes.c_uint64()
    job = ctypes.c_void_p()
    try:
        assert lib.flatgfa_crush(None, ctypes.byref(out)) == -1
        assert lib.flatgfa_crush(g._h, None) == -1
        assert "flatgfa_crush" in _lib.last_error()
        assert lib.flatgfa_dev_crush_count(None, None, 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(n)) == -1
        assert lib.flatgfa_dev_crush_count(None, None, 0, 0, None, None, ctypes.byref(job), None, ctypes.byref(n)) == -1
        # segments without spans, a pool without bytes
        assert lib.flatgfa_dev_crush_count(None, None, 0, 3, None, None, ctypes.byref(job), ctypes.byref(n), ctypes.byref(n)) == -1
        assert lib.flatgfa_dev_crush_count(None, None, 5, 0, None, None, ctypes.byref(job), ctypes.byref(n), ctypes.byref(n)) == -1
        assert job.value is None
        assert lib.flatgfa_dev_crush_fill(None, None, None, None) == -1
        lib.flatgfa_dev_crush_free(None)
    finally:
        g.close()


def test_cli_usage_error_exits_2(tmp_path):
    gfa = tmp_path / "g.gfa"
    gfa.write_bytes(TEXT)
    r = subprocess.run([FGFA, "-I", str(gfa), "crush", "-x"], capture_output=True, timeout=120, env=dict(os.environ, FLATGFA_NO_WARM="1"))
    assert r.returncode == 2 and b"usage: fgfa crush" in r.stderr and r.stdout == b""


def test_the_model_refuses_what_the_handle_refuses():
    with pytest.raises(IndexError):
        cm.crush(cs.pools(np.frombuffer(b"ANNA", np.uint8).copy(), [(0, 4), (2, 5)]))
