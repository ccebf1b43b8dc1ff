"""What BED intersection says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every GPU-only route
says (skipped where a device is visible).  Argument errors, parse errors and the size refusals are decided before any device
work, so they are answered the same with and without a device, and are tested here; so are the CLI's usage errors."""
import ctypes
import os
import subprocess

import pytest

import bed_model as bm
import pollen_amd as pa
from conftest import ROOT
from pollen_amd import _lib

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
MESSAGE = "no HIP device is visible; bed has no CPU fallback"
NO_WARM = dict(os.environ, FLATGFA_NO_WARM="1")
A, B = b"x\t1\t5\n", b"x\t2\t9\n"
MALFORMED = {"no start": b"x\n", "no end": b"x\t1\n", "end is no number": b"x\t1\tq\n", "an empty line": b"x\t1\t2\n\n"}


def no_device():
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")


def test_no_device_messages(tmp_path):
    no_device()
    for call in (lambda: pa.bed_intersect(A, B), lambda: pa.bed_intersect_count(A, B), lambda: pa.bed_intersect_stream(A, B, lambda p: None)):
        with pytest.raises(pa.FlatGFAError) as e:
            call()
        assert e.value.code == -3 and _lib.last_error() == MESSAGE  # FLATGFA_ERR_NO_DEVICE
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(A)
    fb.write_bytes(B)
    with pytest.raises(pa.FlatGFAError) as e:
        pa.bed_intersect(fa, str(fb))  # (paths)
    assert e.value.code == -3


def test_cli_without_a_device(tmp_path):
    no_device()
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(A)
    fb.write_bytes(B)
    r = subprocess.run([FGFA, "bed", "-a", str(fa), "-b", str(fb)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and MESSAGE.encode() in r.stderr and r.stdout == b""


def depth_table_answer(bed: bytes):
    """the code and sentence flatgfa_bed_depth_table gives for the same text"""
    with pa.parse_bytes(b"S\t1\tA\nP\tx\t1+\t*\n") as g:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        rc = _lib.lib().flatgfa_bed_depth_table(g._h, bed, len(bed), ctypes.byref(p), ctypes.byref(n))
        return rc, _lib.last_error()


@pytest.mark.parametrize("name", list(MALFORMED))
@pytest.mark.parametrize("side", ["a", "b"])
def test_a_parse_error_is_the_depth_tables(name, side):
    # (with or without a device: the texts are parsed first)
    bad = MALFORMED[name]
    with pytest.raises(bm.BedError) as model:
        bm.parse(bad)
    want = depth_table_answer(bad)
    assert want[0] == -2 and want[1] == str(model.value)
    a, b = (bad, B) if side == "a" else (A, bad)
    lib = _lib.lib()
    text, n = ctypes.c_void_p(), ctypes.c_size_t(7)
    assert (lib.flatgfa_bed_intersect(a, len(a), b, len(b), ctypes.byref(text), ctypes.byref(n)), _lib.last_error()) == want
    assert text.value is None and n.value == 0

    def sink(ctx, p, m):
        raise AssertionError("delivered")
    assert (lib.flatgfa_bed_intersect_stream(a, len(a), b, len(b), _lib.SINK_T(sink), None), _lib.last_error()) == want
    u = [ctypes.c_uint64(9) for _ in range(4)]
    assert (lib.flatgfa_bed_intersect_count(a, len(a), b, len(b), *[ctypes.byref(x) for x in u]), _lib.last_error()) == want
    assert [x.value for x in u] == [0, 0, 0, 0]
    with pytest.raises(pa.FlatGFAError) as e:
        pa.bed_intersect(a, b)
    assert e.value.code == -2


@pytest.mark.parametrize("side", ["a", "b"])
def test_a_text_of_2_to_the_32_bytes_is_refused_before_it_is_read(side):
    """The length is checked first: the buffer is a few bytes at the end of a mapped page with nothing mapped behind it, so a
    parser that believed the length would run off it."""
    import mmap
    page = mmap.PAGESIZE
    m = mmap.mmap(-1, 2 * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(m))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + page, page, 0) == 0  # PROT_NONE behind the text
    m[page - len(A):page] = A  # (no newline follows inside the readable page)
    small = ctypes.c_void_p(base + page - len(A))
    lib = _lib.lib()
    text, n = ctypes.c_void_p(), ctypes.c_size_t()
    u = [ctypes.c_uint64() for _ in range(4)]

    def sink(ctx, p, k):
        raise AssertionError("delivered")
    cb = _lib.SINK_T(sink)
    for length in (1 << 32, (1 << 32) + 5, 1 << 40):
        args = (small, length, B, len(B)) if side == "a" else (B, len(B), small, length)
        args = tuple(ctypes.cast(x, ctypes.c_char_p) if isinstance(x, ctypes.c_void_p) else x for x in args)
        for rc in (lib.flatgfa_bed_intersect(*args, ctypes.byref(text), ctypes.byref(n)), lib.flatgfa_bed_intersect_stream(*args, cb, None),
                   lib.flatgfa_bed_intersect_count(*args, *[ctypes.byref(x) for x in u])):
            assert rc == -2 and _lib.last_error().startswith("bed: ")  # FLATGFA_ERR_BOUNDS
        assert text.value is None
    libc.mprotect(base + page, page, 3)


def test_argument_errors_need_no_device():
    lib = _lib.lib()
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    u = [ctypes.c_uint64() for _ in range(4)]
    r = [ctypes.byref(x) for x in u]

    def sink(ctx, q, m):
        return 0
    cb = _lib.SINK_T(sink)
    calls = [
        lambda: lib.flatgfa_bed_intersect(None, 5, B, len(B), ctypes.byref(p), ctypes.byref(n)),
        lambda: lib.flatgfa_bed_intersect(A, len(A), None, 5, ctypes.byref(p), ctypes.byref(n)),
        lambda: lib.flatgfa_bed_intersect(A, len(A), B, len(B), None, ctypes.byref(n)),
        lambda: lib.flatgfa_bed_intersect(A, len(A), B, len(B), ctypes.byref(p), None),
        lambda: lib.flatgfa_bed_intersect_stream(None, 5, B, len(B), cb, None),
        lambda: lib.flatgfa_bed_intersect_stream(A, len(A), None, 5, cb, None),
        lambda: lib.flatgfa_bed_intersect_stream(A, len(A), B, len(B), None, None),
        lambda: lib.flatgfa_bed_intersect_count(None, 5, B, len(B), *r),
        lambda: lib.flatgfa_bed_intersect_count(A, len(A), None, 5, *r),
        lambda: lib.flatgfa_bed_intersect_count(A, len(A), B, len(B), None, r[1], r[2], r[3]),
        lambda: lib.flatgfa_bed_intersect_count(A, len(A), B, len(B), r[0], None, r[2], r[3]),
        lambda: lib.flatgfa_bed_intersect_count(A, len(A), B, len(B), r[0], r[1], None, r[3]),
        lambda: lib.flatgfa_bed_intersect_count(A, len(A), B, len(B), r[0], r[1], r[2], None),
        lambda: lib.flatgfa_dev_bed_begin(None, None, None, 0, None, None, None, 0, 0, 0, None, None, r[0], r[1], r[2]),
        lambda: lib.flatgfa_dev_bed_begin(None, None, None, 0, None, None, None, 0, 0, 0, None, ctypes.byref(p), None, r[1], r[2]),
        lambda: lib.flatgfa_dev_bed_begin(None, None, None, 3, None, None, None, 0, 0, 0, None, ctypes.byref(p), r[0], r[1], r[2]),  # entries without arrays
        lambda: lib.flatgfa_dev_bed_round(None, 0, None, None, None, None, r[0]),
    ]
    for k, call in enumerate(calls):
        assert call() == -1, k  # FLATGFA_ERR_ARG
        assert "NULL" in _lib.last_error(), k
        assert p.value is None, k
    lib.flatgfa_dev_bed_free(None)


@pytest.mark.parametrize("args", [[], ["-a", "A"], ["-b", "B"], ["-a", "A", "-b"], ["-a", "A", "-b", "B", "MORE"], ["-a", "A", "-a", "A", "-b", "B"],
                                  ["A", "B"]], ids=lambda a: " ".join(a) or "none")
def test_cli_usage_errors_exit_2(tmp_path, args):
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(A)
    fb.write_bytes(B)
    args = [str(fa) if x == "A" else str(fb) if x == "B" else x for x in args]
    r = subprocess.run([FGFA, "bed"] + args, capture_output=True, timeout=120, stdin=subprocess.DEVNULL, env=NO_WARM)
    assert r.returncode == 2 and b"usage: fgfa bed -a FILE -b FILE" in r.stderr and r.stdout == b""


def test_cli_does_not_read_stdin(tmp_path):
    # a graph command without -i / -I reads stdin to its end; this one never looks at it
    fa, fb = tmp_path / "a.bed", tmp_path / "b.bed"
    fa.write_bytes(b"x\t1\n")
    fb.write_bytes(B)
    rd, wr = os.pipe()  # the write end stays open: a read of stdin would not return
    try:
        r = subprocess.run([FGFA, "bed", "-a", str(fa), "-b", str(fb)], capture_output=True, timeout=60, stdin=rd, env=NO_WARM)
        assert r.returncode == 1 and r.stdout == b"" and b"BED: line ends after the start column" in r.stderr
        r = subprocess.run([FGFA, "bed"], capture_output=True, timeout=60, stdin=rd, env=NO_WARM)
        assert r.returncode == 2
    finally:
        os.close(rd)
        os.close(wr)


@pytest.mark.parametrize("missing", ["a", "b"])
def test_a_missing_file(tmp_path, missing):
    f = tmp_path / "f.bed"
    f.write_bytes(A)
    a, b = (tmp_path / "none", f) if missing == "a" else (f, tmp_path / "none")
    r = subprocess.run([FGFA, "bed", "-a", str(a), "-b", str(b)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL, env=NO_WARM)
    assert r.returncode == 1 and b"cannot open" in r.stderr and r.stdout == b""
