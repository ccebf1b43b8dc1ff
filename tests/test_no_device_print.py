"""What the device GFA printer says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every
GPU-only route says (tests/test_no_device_messages.py).  Argument errors, and what stops the host printer -- the six
`print:` errors -- are answered before any device is asked for.  The device cases are skipped where one is visible."""
import ctypes
import os
import subprocess

import pytest

import pollen_amd as pa
import print_shapes as ps
from conftest import ROOT
from pollen_amd import _lib
from test_print_model import ERRORS, load

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
TEXT = ps.HANDMADE["plain"]
MESSAGE = "no HIP device is visible; the device GFA printer has no CPU fallback"

ROUTES = {
    "bytes": lambda g, tmp: g.gfa_bytes(),
    "text": lambda g, tmp: g.gfa_text_device(),
    "stream": lambda g, tmp: g.gfa_stream(lambda b: None),
    "file": lambda g, tmp: g.write_gfa_device(str(tmp / "out.gfa")),
}


@pytest.mark.parametrize("what", list(ROUTES))
def test_no_device_message(what, tmp_path):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pa.parse_bytes(TEXT) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            ROUTES[what](g, tmp_path)
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == MESSAGE
        assert not os.path.exists(tmp_path / "out.gfa")
        assert g.gfa_text() == TEXT  # the host printer needs none


def test_no_device_cli(tmp_path):
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(TEXT)
    for extra in ([], ["-O", str(tmp_path / "out.gfa")]):
        r = subprocess.run([FGFA, "-I", str(gfa), "print", *extra], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and MESSAGE.encode() in r.stderr
        assert not os.path.exists(tmp_path / "out.gfa")
    # a bare fgfa stays on the host printer
    r = subprocess.run([FGFA, "-I", str(gfa)], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == TEXT


def test_cli_usage(tmp_path):
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(TEXT)
    for bad in (["print", "extra"], ["print", "-O"], ["print", "-x", "y"]):
        r = subprocess.run([FGFA, "-I", str(gfa), *bad], capture_output=True, timeout=120)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr == b"usage: fgfa [-i FILE | -I FILE] print\n"


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    sink = _lib.SINK_T(lambda ctx, p, n: 0)
    p, n, b = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
    with pa.parse_bytes(TEXT) as g:
        assert lib.flatgfa_print_gfa_bytes(None, ctypes.byref(b)) == -1
        assert lib.flatgfa_print_gfa_bytes(g._h, None) == -1
        assert lib.flatgfa_print_gfa_device(None, ctypes.byref(p), ctypes.byref(n)) == -1
        assert lib.flatgfa_print_gfa_device(g._h, None, ctypes.byref(n)) == -1
        assert lib.flatgfa_print_gfa_device(g._h, ctypes.byref(p), None) == -1
        assert lib.flatgfa_print_gfa_stream(None, sink, None) == -1
        assert lib.flatgfa_print_gfa_stream(g._h, None, None) == -1
        assert "flatgfa_print_gfa_stream: NULL argument" == _lib.last_error()


@pytest.mark.parametrize("message", list(ERRORS))
def test_print_errors_need_no_device(message, tmp_path):
    """With print_gfa's code and sentence, whether or not there is a device."""
    with load(ERRORS[message](), tmp_path) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            g.gfa_text()
        want = (e.value.code, _lib.last_error())
        assert want == (-2, message)
        calls = []
        for call in (g.gfa_bytes, g.gfa_text_device, lambda: g.gfa_stream(calls.append),
                     lambda: g.write_gfa_device(str(tmp_path / "out.gfa"))):
            with pytest.raises(pa.FlatGFAError) as e:
                call()
            assert (e.value.code, _lib.last_error()) == want
        assert calls == [] and not os.path.exists(tmp_path / "out.gfa")
        r = subprocess.run([FGFA, "-i", str(tmp_path / "shape.flatgfa"), "print", "-O", str(tmp_path / "cli.gfa")], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and message.encode() in r.stderr
        assert not os.path.exists(tmp_path / "cli.gfa")


def test_first_error_in_line_order(tmp_path):
    """A bad kind on line 1 is met before the missing path of line 2; a missing segment on line 0 before both."""
    for order, message in (([1, 4, 2, 2], "print: bad line kind"), ([1, 2, 2, 4], "print: too few paths"),
                           ([1, 1, 1, 1, 4], "print: too few segments"), ([3, 3, 0, 3], "print: too few links")):
        with load(ps.order_of(TEXT, order), tmp_path) as g:
            with pytest.raises(pa.FlatGFAError) as e:
                g.gfa_bytes()
            assert (e.value.code, _lib.last_error()) == (-2, message)
            with pytest.raises(pa.FlatGFAError):
                g.gfa_text()
            assert _lib.last_error() == message
