"""What flip says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only route says.  Skipped
where a device is visible.  Spans that leave their pools, the laid-out steps' count and the argument errors are decided before
any device work, so they are answered the same with and without a device, and are tested here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flip_model as fm
import flip_shapes as fs
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

TEXT = b"S\t1\tAA\nS\t2\tCC\nS\t3\tGGG\nP\tp0\t1+,2-\t*\nP\tp1\t3-,2-,1+\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t4M\n"
MESSAGE = "no HIP device is visible; flip has no CPU fallback"
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def test_no_device_message():
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    try:
        for call in (g.flip, g.flip_count):
            with pytest.raises(pa.FlatGFAError) as e:
                call()
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
    args = [FGFA, "-I", str(gfa)] + (["-o", str(out)] if how == "-o" else []) + ["flip"]
    r = subprocess.run(args, capture_output=True, timeout=120)
    assert r.returncode == 1 and MESSAGE.encode() in r.stderr and r.stdout == b"" and not out.exists()


def poke(g, pool, index, words):
    """Element `index` of a heap handle's pool gets these u32 words, behind the library's back: the loaders refuse a file
    with such a span, so this is the one way a handle comes to hold it."""
    data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, fo.POOL_ORDER.index(pool), ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
    assert index < n.value and es.value == 4 * len(words)
    dst = ctypes.cast(data.value + es.value * index, ctypes.POINTER(ctypes.c_uint32))
    for k, w in enumerate(words):
        dst[k] = w


BAD = {
    "a path one past the steps": ("paths", 1, [2, 4, 3, 6, 0, 0], "flip: path 1 has a step span outside the steps pool"),
    "a path that ends before it begins": ("paths", 0, [0, 2, 2, 1, 0, 0], "flip: path 0 has a step span outside the steps pool"),
    "a name one past name_data": ("paths", 1, [2, 5, 2, 5, 0, 0], "flip: path 1 has a name span outside name_data"),
    "a segment one past seq_data": ("segs", 2, [3, 0, 4, 8, 0, 0], "flip: segment 2 has a sequence span outside seq_data"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_a_bad_span_is_refused_before_any_device_work(name):
    # (with or without a device: BOUNDS, never NO_DEVICE -- the spans are checked first)
    g = pa.parse_bytes(TEXT)
    try:
        pool, index, words, message = BAD[name]
        poke(g, pool, index, words)
        for call in (g.flip, g.flip_count):
            with pytest.raises(pa.FlatGFAError) as e:
                call()
            assert e.value.code == -2  # FLATGFA_ERR_BOUNDS
            assert _lib.last_error() == message
    finally:
        g.close()


def test_more_laid_out_steps_than_2_to_the_32_is_refused_before_any_device_work():
    # 65537 paths that all walk the same 65536 steps
    p = fs.graph([1], [], [], spans=[(0, 1 << 16)] * ((1 << 16) + 1), steps=np.full(1 << 16, fs.h(0, True), np.uint32))
    with fm.handle_of(p) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            g.flip()
        assert e.value.code == -6 and _lib.last_error() == "flip: the paths hold more than 2^32 - 1 steps"  # FLATGFA_ERR_TOO_LARGE


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    g = pa.parse_bytes(TEXT)
    out, job = ctypes.c_void_p(), ctypes.c_void_p()
    n = ctypes.c_uint64()
    try:
        assert lib.flatgfa_flip(None, ctypes.byref(out)) == -1
        assert lib.flatgfa_flip(g._h, None) == -1
        assert "flatgfa_flip" in _lib.last_error()
        assert lib.flatgfa_flip_count(None, ctypes.byref(n), ctypes.byref(n)) == -1
        args = [None, 0, None, None, 0, 0, None, 0, None, 0, None, 0, 0, None]
        assert lib.flatgfa_dev_flip_count(*args, None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == -1
        assert lib.flatgfa_dev_flip_count(*args, ctypes.byref(job), None, ctypes.byref(n), ctypes.byref(n)) == -1
        assert lib.flatgfa_dev_flip_count(*args, ctypes.byref(job), ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == -1  # (no path starts)
        assert job.value is None
        assert lib.flatgfa_dev_flip_fill(None, None, None, None, None) == -1
        lib.flatgfa_dev_flip_free(None)
    finally:
        g.close()


def test_cli_usage_error_exits_2(tmp_path):
    gfa = tmp_path / "g.gfa"
    gfa.write_bytes(TEXT)
    r = subprocess.run([FGFA, "-I", str(gfa), "flip", "-x"], capture_output=True, timeout=120, env=dict(os.environ, FLATGFA_NO_WARM="1"))
    assert r.returncode == 2 and b"usage: fgfa flip" in r.stderr and r.stdout == b""


def test_the_model_refuses_what_the_handle_refuses():
    p = fs.graph([2, 2, 3], [[0, 3], [5, 3, 0]], [(0, 2, [0])])
    p.paths[1] = (2, 4, 3, 6, 0, 0)
    with pytest.raises(IndexError):
        fm.flip(p)
