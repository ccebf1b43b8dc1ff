"""What the packed-sequence codec says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only
route says (skipped where a device is visible).  The header checks and the argument errors are decided before any device work,
so they are answered the same with and without a device, and are tested here; so are the CLI's usage errors."""
import ctypes
import os
import subprocess

import pytest

import pollen_amd as pa
import seq_model as sm
from conftest import ROOT
from pollen_amd import _lib
from seq_shapes import ACCEPTED, KNOWN, REFUSED

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
EXPORT_MESSAGE = "no HIP device is visible; seq-export has no CPU fallback"
IMPORT_MESSAGE = "no HIP device is visible; seq-import has no CPU fallback"
NO_WARM = dict(os.environ, FLATGFA_NO_WARM="1")


def no_device():
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")


def test_no_device_messages(tmp_path):
    no_device()
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_export(b"ACTGG\n")
    assert e.value.code == -3 and _lib.last_error() == EXPORT_MESSAGE  # FLATGFA_ERR_NO_DEVICE
    out = tmp_path / "p"
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_export_file(b"ACTGG\n", out)
    assert e.value.code == -3 and _lib.last_error() == EXPORT_MESSAGE and not out.exists()
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_import(KNOWN)
    assert e.value.code == -3 and _lib.last_error() == IMPORT_MESSAGE


def test_cli_without_a_device(tmp_path):
    no_device()
    text, packed, out = tmp_path / "t", tmp_path / "p", tmp_path / "o"
    text.write_bytes(b"ACTGG\n")
    packed.write_bytes(KNOWN)
    r = subprocess.run([FGFA, "seq-export", str(text), str(out)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and EXPORT_MESSAGE.encode() in r.stderr and r.stdout == b"" and not out.exists()
    r = subprocess.run([FGFA, "seq-import", str(packed)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and IMPORT_MESSAGE.encode() in r.stderr and r.stdout == b""


@pytest.mark.parametrize("name", list(REFUSED))
def test_a_malformed_header_is_refused_before_any_device_work(name):
    # (with or without a device: PARSE, never NO_DEVICE -- the header is checked first)
    file = REFUSED[name]
    with pytest.raises(sm.SeqError):
        sm.packed_info(file)
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_packed_info(file)
    assert e.value.code == -7 and _lib.last_error().startswith("seq-import: ")  # FLATGFA_ERR_PARSE
    text, n = ctypes.c_void_p(), ctypes.c_size_t(7)
    assert _lib.lib().flatgfa_seq_import(file, len(file), ctypes.byref(text), ctypes.byref(n)) == -7
    assert text.value is None and n.value == 0
    assert _lib.last_error().startswith("seq-import: ")

    def sink(ctx, p, m):
        raise AssertionError("delivered")
    assert _lib.lib().flatgfa_seq_import_stream(file, len(file), _lib.SINK_T(sink), None) == -7


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_packed_info_needs_no_device(name):
    file, want = ACCEPTED[name]
    assert pa.seq_packed_info(file) == (len(want), 25) == sm.packed_info(file)


def test_cli_refuses_a_malformed_file(tmp_path):
    packed = tmp_path / "p"
    packed.write_bytes(REFUSED["wrong magic"])
    r = subprocess.run([FGFA, "seq-import", str(packed)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL, env=NO_WARM)
    assert r.returncode == 1 and b"seq-import: the magic number is 19" in r.stderr and r.stdout == b""


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    p, n, u = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()

    def sink(ctx, q, m):
        return 0
    cb = _lib.SINK_T(sink)
    calls = [
        lambda: lib.flatgfa_seq_export(None, 5, ctypes.byref(p), ctypes.byref(n)),
        lambda: lib.flatgfa_seq_export(b"ACTGG", 5, None, ctypes.byref(n)),
        lambda: lib.flatgfa_seq_export(b"ACTGG", 5, ctypes.byref(p), None),
        lambda: lib.flatgfa_seq_export_file(None, 5, b"/nonexistent/x"),
        lambda: lib.flatgfa_seq_export_file(b"ACTGG", 5, None),
        lambda: lib.flatgfa_seq_import(None, 28, ctypes.byref(p), ctypes.byref(n)),
        lambda: lib.flatgfa_seq_import(KNOWN, 28, None, ctypes.byref(n)),
        lambda: lib.flatgfa_seq_import(KNOWN, 28, ctypes.byref(p), None),
        lambda: lib.flatgfa_seq_import_stream(None, 28, cb, None),
        lambda: lib.flatgfa_seq_import_stream(KNOWN, 28, None, None),
        lambda: lib.flatgfa_seq_packed_info(None, 28, ctypes.byref(u), ctypes.byref(u)),
        lambda: lib.flatgfa_seq_packed_info(KNOWN, 28, None, ctypes.byref(u)),
        lambda: lib.flatgfa_seq_packed_info(KNOWN, 28, ctypes.byref(u), None),
        lambda: lib.flatgfa_dev_seq_pack_count(None, 0, None, None, ctypes.byref(u)),
        lambda: lib.flatgfa_dev_seq_pack_count(None, 0, None, ctypes.byref(p), None),
        lambda: lib.flatgfa_dev_seq_pack_count(None, 5, None, ctypes.byref(p), ctypes.byref(u)),  # bytes without a text
        lambda: lib.flatgfa_dev_seq_pack_fill(None, -1, None, None),
        lambda: lib.flatgfa_dev_seq_unpack(None, 5, None, None),
    ]
    for k, call in enumerate(calls):
        assert call() == -1, k  # FLATGFA_ERR_ARG
        assert p.value is None, k
    assert "NULL" in _lib.last_error()
    lib.flatgfa_dev_seq_pack_free(None)
    # n == 0 with NULL is no argument error: the header check answers
    assert lib.flatgfa_seq_packed_info(None, 0, ctypes.byref(u), ctypes.byref(u)) == -7


@pytest.mark.parametrize("args", [["seq-export"], ["seq-export", "IN"], ["seq-export", "IN", "OUT", "MORE"], ["seq-import"],
                                  ["seq-import", "IN", "MORE"]], ids=" ".join)
def test_cli_usage_errors_exit_2(tmp_path, args):
    text, out = tmp_path / "t", tmp_path / "o"
    text.write_bytes(b"ACTGG\n")
    args = [str(text) if a == "IN" else str(out) if a == "OUT" else a for a in args]
    r = subprocess.run([FGFA] + args, capture_output=True, timeout=120, stdin=subprocess.DEVNULL, env=NO_WARM)
    usage = b"usage: fgfa seq-export INPUT OUTPUT" if args[0] == "seq-export" else b"usage: fgfa seq-import FILE"
    assert r.returncode == 2 and usage in r.stderr and r.stdout == b"" and not out.exists()


def test_cli_does_not_read_stdin(tmp_path):
    # a graph command without -i / -I reads stdin to its end; these two never look at it
    packed = tmp_path / "p"
    packed.write_bytes(REFUSED["data cut short"])
    rd, wr = os.pipe()  # the write end stays open: a read of stdin would not return
    try:
        r = subprocess.run([FGFA, "seq-import", str(packed)], capture_output=True, timeout=60, stdin=rd, env=NO_WARM)
        assert r.returncode == 1 and r.stdout == b"" and b"seq-import: the header promises 3 bytes and 2 follow it" in r.stderr
        r = subprocess.run([FGFA, "seq-export"], capture_output=True, timeout=60, stdin=rd, env=NO_WARM)
        assert r.returncode == 2
    finally:
        os.close(rd)
        os.close(wr)


def test_a_missing_input_file(tmp_path):
    out = tmp_path / "o"
    r = subprocess.run([FGFA, "seq-export", str(tmp_path / "none"), str(out)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL, env=NO_WARM)
    assert r.returncode == 1 and b"cannot open" in r.stderr and not out.exists()
