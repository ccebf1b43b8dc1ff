"""The packed-sequence codec on the GPU against tests/seq_model.py, byte for byte: through the host route, through the device
entries and through `fgfa`.  Lengths, whitespace, refusals, the reader's cases, the host route's chunks, random round trips.
The kernels' seams are in tests/test_gpu_seq_geometry.py.  Run with -m gpu."""
import ctypes
import subprocess

import numpy as np
import pytest

import pollen_amd as pa
import seq_gpu as sg
import seq_model as sm
import seq_shapes as ss
from pollen_amd import _lib
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
T = sm.TILE


def test_known_answer_three_ways(tmp_path):
    assert pa.seq_export(b"ACTGG\n") == ss.KNOWN
    assert pa.seq_import(ss.KNOWN) == b"ACTGG"
    packed = sg.check_device(b"ACTGG\n")
    assert packed.cpu().numpy().tobytes() == ss.KNOWN[25:]
    sg.check_cli(b"ACTGG\n", tmp_path)
    assert (tmp_path / "out.packed").read_bytes() == ss.KNOWN
    out = tmp_path / "by_file"
    pa.seq_export_file(b"ACTGG\n", out)
    assert out.read_bytes() == ss.KNOWN and pa.seq_import_file(out) == b"ACTGG"


@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 32, 33])
def test_lengths(n, tmp_path):
    seq = bytes(ss.bases(n, n))
    for text in (seq, seq + b"\n", b"\n" + seq):
        sg.check_host(text, n)
        sg.check_device(text, n)
    sg.check_cli(seq + b"\n", tmp_path, n)
    assert len(pa.seq_export(seq)) == 25 + (n + 1) // 2


@pytest.mark.parametrize("text", [b"", b" ", b" \t\n\x0c\r" * 9], ids=["empty", "one space", "all five"])
def test_whitespace_only(text, tmp_path):
    assert pa.seq_export(text) == ss.EMPTY
    assert pa.seq_import(ss.EMPTY) == b""
    sg.check_device(text)
    sg.check_cli(text, tmp_path)
    assert (tmp_path / "out.packed").read_bytes() == ss.EMPTY  # ... and its import printed one newline


@pytest.mark.parametrize("ws", list(sm.WHITESPACE), ids=lambda b: f"0x{b:02x}")
def test_each_whitespace_byte_is_dropped(ws):
    text = bytes([ws]) + b"AC" + bytes([ws, ws]) + b"G" + bytes([ws])
    assert pa.seq_export(text) == sm.export(b"ACG")
    sg.check_device(text)


@pytest.mark.parametrize("bad", [0x0B, ord("a"), ord("N"), 0x00, 0xFF], ids=lambda b: f"0x{b:02x}")
def test_a_byte_that_is_no_nucleotide_is_refused(bad, tmp_path):
    text = b"ACGT \n" + bytes([bad]) + b"AC"
    message = sg.bad_byte_message(bad, 6)
    assert sg.export_error(text) == (-7, message)  # FLATGFA_ERR_PARSE
    assert sg.pack_error(sg.to_device(text)) == (-7, message)
    # nothing is written: no image, no job, no file
    p, n = ctypes.c_void_p(), ctypes.c_size_t(3)
    assert _lib.lib().flatgfa_seq_export(text, len(text), ctypes.byref(p), ctypes.byref(n)) == -7 and p.value is None and n.value == 0
    job, u = ctypes.c_void_p(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_dev_seq_pack_count(sg.to_device(text).data_ptr(), len(text), None, ctypes.byref(job), ctypes.byref(u)) == -7
    assert job.value is None
    src, out = tmp_path / "t", tmp_path / "p"
    src.write_bytes(text)
    with pytest.raises(pa.FlatGFAError):
        pa.seq_export_file(text, out)
    assert not out.exists()
    r = subprocess.run([sg.FGFA, "seq-export", str(src), str(out)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and message.encode() in r.stderr and r.stdout == b"" and not out.exists()


def test_a_bad_byte_as_the_very_last_byte():
    for n in (1, 16, 17, T, T + 1):
        text = bytes(ss.bases(n - 1, n)) + b"N"
        assert sg.export_error(text) == (-7, sg.bad_byte_message(ord("N"), n - 1))
        assert sg.pack_error(sg.to_device(text)) == (-7, sg.bad_byte_message(ord("N"), n - 1))


# ---- the reader ----
@pytest.mark.parametrize("name", list(ss.ACCEPTED))
def test_import_accepts(name, tmp_path):
    file, want = ss.ACCEPTED[name]
    assert pa.seq_import(file) == want == sm.import_(file)
    got = []

    def sink(ctx, p, n):
        got.append(ctypes.string_at(p, n))
        return 0
    assert _lib.lib().flatgfa_seq_import_stream(file, len(file), _lib.SINK_T(sink), None) == 0
    assert b"".join(got) == want
    path = tmp_path / "p"
    path.write_bytes(file)
    r = subprocess.run([sg.FGFA, "seq-import", str(path)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stdout == want + b"\n"


@pytest.mark.parametrize("name", list(ss.REFUSED))
def test_import_refuses(name):
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_import(ss.REFUSED[name])
    assert e.value.code == -7


def image_of(data: bytes, n_bases: int) -> bytes:
    return sm.header(n_bases) + data


@pytest.mark.parametrize("n", [7, 64, 65, 4 * T + 3])
def test_import_a_bad_nibble_names_the_first_base(n, tmp_path):
    data = bytearray(sm.pack_codes(sm.codes_of(ss.bases(n, n))))
    # the unused last high nibble may hold anything
    if n & 1:
        data[-1] |= 0xF0
        assert pa.seq_import(image_of(bytes(data), n)) == bytes(ss.bases(n, n))
        assert pdev.seq_unpack(sg.to_device(bytes(data)), n).cpu().numpy().tobytes() == bytes(ss.bases(n, n))
    # two bad nibbles: a high one at base `first`, a low one later
    first, second = (n // 3) | 1, (n // 3 + 3) & ~1
    assert first < second < n
    data[first // 2] = (data[first // 2] & 0x0F) | 0x40
    data[second // 2] = (data[second // 2] & 0xF0) | 0x0C
    message = f"seq-import: nibble 4 at base {first} is not a nucleotide"
    with pytest.raises(sm.SeqError) as m:
        sm.import_(image_of(bytes(data), n))
    assert str(m.value) == message
    with pytest.raises(pa.FlatGFAError) as e:
        pa.seq_import(image_of(bytes(data), n))
    assert e.value.code == -7 and _lib.last_error() == message
    with pytest.raises(pa.FlatGFAError) as e:
        pdev.seq_unpack(sg.to_device(bytes(data)), n)
    assert e.value.code == -7 and _lib.last_error() == message
    # nothing is delivered
    got = []

    def sink(ctx, p, k):
        got.append(k)
        return 0
    file = image_of(bytes(data), n)
    assert _lib.lib().flatgfa_seq_import_stream(file, len(file), _lib.SINK_T(sink), None) == -7 and not got
    path = tmp_path / "p"
    path.write_bytes(file)
    r = subprocess.run([sg.FGFA, "seq-import", str(path)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and message.encode() in r.stderr and r.stdout == b""


def test_a_sink_that_stops():
    def sink(ctx, p, n):
        return 1
    assert _lib.lib().flatgfa_seq_import_stream(ss.KNOWN, len(ss.KNOWN), _lib.SINK_T(sink), None) == -5  # FLATGFA_ERR_IO


# ---- the host route's chunks ----
@pytest.mark.parametrize("chunk", ss.CHUNKS)
@pytest.mark.parametrize("name", list(ss.CHUNK_TEXTS))
def test_export_chunks_do_not_show(name, chunk, monkeypatch):
    text = ss.CHUNK_TEXTS[name]
    want = sm.export(text)
    assert sm.export_chunked(text, chunk) == want
    monkeypatch.setenv("FLATGFA_SEQ_CHUNK_BYTES", str(chunk))
    assert pa.seq_export(text) == want
    assert pa.seq_import(want) == sm.import_(want)


@pytest.mark.parametrize("chunk", [3, 7, 4097])
def test_export_chunks_on_tiles_of_text(chunk, monkeypatch):
    # chunks of 4097 bytes over a few tiles; the small ones over a text that they cut some dozens of times
    text = bytes(ss.sprinkled(3 * T + 5 if chunk == 4097 else 260, 0.3, chunk))
    want = sm.export(text)
    monkeypatch.setenv("FLATGFA_SEQ_CHUNK_BYTES", str(chunk))
    assert pa.seq_export(text) == want
    assert pa.seq_import(want) == sm.import_(want)
    got = []

    def sink(ctx, p, n):
        got.append(ctypes.string_at(p, n))
        return 0
    assert _lib.lib().flatgfa_seq_import_stream(want, len(want), _lib.SINK_T(sink), None) == 0
    assert b"".join(got) == sm.import_(want) and max(map(len, got)) <= chunk


@pytest.mark.parametrize("chunk", [1, 7])
def test_a_bad_byte_in_a_later_chunk_names_its_offset_in_the_text(chunk, monkeypatch):
    text = b"AC G\nTT" + b"x" + b"ACn"
    monkeypatch.setenv("FLATGFA_SEQ_CHUNK_BYTES", str(chunk))
    assert sg.export_error(text) == (-7, sg.bad_byte_message(ord("x"), 7))
    data = bytearray(sm.export(b"ACGTACGTACGTACGTACG"))
    data[25 + 6] |= 0x80  # base 13
    data[25 + 8] |= 0x08  # base 16
    with pytest.raises(pa.FlatGFAError):
        pa.seq_import(bytes(data))
    assert _lib.last_error() == "seq-import: nibble 9 at base 13 is not a nucleotide"


# ---- random ----
@pytest.mark.parametrize("seed", range(12))
def test_random_round_trip(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 4 * T + 1)) if seed else 4 * T
    text = ss.sprinkled(n, float(rng.uniform(0, 0.3)), seed)
    sg.check_device(text, seed)
    sg.check_host(text, seed)
