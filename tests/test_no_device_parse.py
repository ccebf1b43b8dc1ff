"""What the device GFA parser says on a machine without a HIP device: NULL and the sentence every GPU-only route says
(tests/test_no_device_messages.py), from the library and from `fgfa -D`.  Argument errors and `fgfa -D` usage are answered
without a device; a bare `fgfa -I` is the host parser's, as before.  The device cases are skipped where one is visible."""
import ctypes
import os
import subprocess

import pytest

import pollen_amd as pa
import parse_shapes as ps
from conftest import ROOT
from pollen_amd import _lib

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
TEXT = ps.HANDMADE["plain"]
MESSAGE = "no HIP device is visible; the device GFA parser has no CPU fallback"


def run(*args, **kw):
    return subprocess.run([FGFA, *args], capture_output=True, timeout=120, **kw)


def test_no_device_message(tmp_path):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(TEXT)
    lib = _lib.lib()
    for call in (lambda: lib.flatgfa_parse_bytes_device(TEXT, len(TEXT), 0), lambda: lib.flatgfa_parse_bytes_device(TEXT, len(TEXT), 1),
                 lambda: lib.flatgfa_parse_bytes_device(b"", 0, 0), lambda: lib.flatgfa_parse_device(os.fsencode(str(gfa)))):
        assert call() is None and _lib.last_error() == MESSAGE
    for call in (lambda: pa.parse_bytes_device(TEXT), lambda: pa.parse_bytes_device(TEXT, stream=True), lambda: pa.parse_device(str(gfa))):
        with pytest.raises(pa.FlatGFAError):
            call()
        assert _lib.last_error() == MESSAGE
    assert pa.parse_bytes(TEXT).gfa_text() == TEXT  # the host parser needs none


def test_no_device_cli(tmp_path):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(TEXT)
    out = tmp_path / "out.flatgfa"
    for r in (run("-D", "-I", str(gfa)), run("-D", input=TEXT), run("-D", "-I", str(gfa), "-o", str(out)), run("-D", "-I", str(gfa), "paths")):
        assert r.returncode == 1 and r.stdout == b"" and MESSAGE.encode() in r.stderr
    assert not out.exists()


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    assert lib.flatgfa_parse_bytes_device(None, 5, 0) is None
    assert _lib.last_error() == "flatgfa_parse_bytes_device: NULL data with a length"
    assert lib.flatgfa_parse_device(None) is None
    assert _lib.last_error() == "flatgfa_parse_device: NULL filename"
    assert lib.flatgfa_parse_device(b"/nonexistent/in.gfa") is None and "cannot open" in _lib.last_error()
    assert lib.flatgfa_parse_device_info(None) == -1
    assert lib.flatgfa_parse_device_times(None) == -1
    if pa.device_count() == 0:  # no call has reached a device: there is nothing to report
        assert lib.flatgfa_parse_device_info((ctypes.c_uint64 * 4)()) == -1


def test_cli_usage_and_the_bare_route(tmp_path):
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(TEXT)
    with pa.parse_bytes(TEXT) as g:
        g.write_flatgfa(str(tmp_path / "in.flatgfa"))
    r = run("-D", "-i", str(tmp_path / "in.flatgfa"))
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"usage: fgfa -D parses GFA text")
    r = run("-D", "-I", str(tmp_path / "missing.gfa"))
    assert r.returncode == 1 and b"cannot open" in r.stderr
    # without -D nothing changes: the host parser, with or without a device
    assert run("-I", str(gfa)).stdout == TEXT and run(input=TEXT).stdout == TEXT
    r = run("-I", str(gfa), "-o", str(tmp_path / "host.flatgfa"))
    assert r.returncode == 0 and (tmp_path / "host.flatgfa").read_bytes() == (tmp_path / "in.flatgfa").read_bytes()
