"""The pack and unpack kernels at their seams (tests/seq_shapes.py): tiles that begin on a high nibble, ranges of tiles that
do, whitespace over whole ranges, pointers off 16-byte alignment, the carry, offsets past 2^32.  Every output byte belongs to one
workgroup, so every test also looks at the bytes beside the output.  Run with -m gpu.

FLATGFA_SEQ_GRID is the job's test hook: fewer workgroups than seq_device.hpp's kSeqGrid, so that a text of a few tiles has
ranges of several tiles; the seams of the library's own grid are run too, on texts of GRID tiles and more."""
import ctypes

import numpy as np
import pytest

import pollen_amd as pa
import seq_gpu as sg
import seq_model as sm
import seq_shapes as ss
from pollen_amd import _lib
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
T, G = sm.TILE, sm.GRID


def raw_pack(text_tensor, carry=-1, out_offset=0, stream=None):
    """The device entries by hand: the packed bytes land out_offset bytes into a room filled with 0x55, 64 spare bytes either side.
    Returns (the room as numpy, where the output begins, n_bases)."""
    import torch
    lib = _lib.lib()
    job, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib.flatgfa_dev_seq_pack_count(text_tensor.data_ptr() if text_tensor.numel() else None, text_tensor.numel(), stream, ctypes.byref(job),
                                        ctypes.byref(n))
    assert rc == 0, _lib.last_error()
    nbytes = (n.value + (carry >= 0) + 1) // 2
    room = torch.full((nbytes + 128 + 16,), 0x55, dtype=torch.uint8, device=text_tensor.device)
    assert room.data_ptr() % 16 == 0
    at = 64 + out_offset
    try:
        assert lib.flatgfa_dev_seq_pack_fill(job, carry, room.data_ptr() + at, stream) == 0, _lib.last_error()
    finally:
        lib.flatgfa_dev_seq_pack_free(job)
    return room.cpu().numpy(), at, n.value


def check_raw(text, carry=-1, in_offset=0, out_offset=0, what=""):
    """Pack of a text that begins in_offset bytes into its tensor, with a carry, into a destination off alignment; the bytes
    against the model's, and not a byte beside them."""
    import torch
    text = sg.as_array(text)
    codes = sm.codes_of(text)
    logical = codes if carry < 0 else np.concatenate([np.array([carry], np.uint8), codes])
    want = sm.pack_codes(logical).tobytes()
    room_in = torch.full((len(text) + 32,), ord("!"), dtype=torch.uint8, device="cuda:0")  # ('!' is no nucleotide: reading beside the text shows)
    assert room_in.data_ptr() % 16 == 0
    room_in[in_offset:in_offset + len(text)] = torch.from_numpy(text.copy()).to("cuda:0")
    got, at, n = raw_pack(room_in[in_offset:in_offset + len(text)], carry, out_offset)
    assert n == len(codes), what
    assert got[at:at + len(want)].tobytes() == want, what
    assert (got[:at] == 0x55).all() and (got[at + len(want):] == 0x55).all(), what


@pytest.mark.parametrize("name", list(ss.TILE_SEAMS))
def test_tile_seams(name, monkeypatch):
    text, grid = ss.TILE_SEAMS[name]()
    if grid is not None:
        monkeypatch.setenv("FLATGFA_SEQ_GRID", str(grid))
    check_raw(text, what=name)
    sg.check_device(text, name)
    sg.check_host(text, name)


@pytest.mark.parametrize("tiles,grid", ss.RANGE_SEAMS_SMALL)
def test_range_seams_on_a_small_grid(tiles, grid, monkeypatch):
    monkeypatch.setenv("FLATGFA_SEQ_GRID", str(grid))
    text = ss.odd_ranges(tiles, grid, seed=tiles)
    check_raw(text, what=(tiles, grid))
    # the same with a text that ends inside its last tile, and with whitespace all over
    check_raw(text[:-(T // 3)], what=(tiles, grid, "ragged"))
    check_raw(ss.sprinkled(tiles * T - 7, 0.3, tiles), what=(tiles, grid, "sprinkled"))


def test_fewer_tiles_than_workgroups():
    check_raw(ss.odd_ranges(3, G, seed=3), what="3 tiles")
    check_raw(ss.sprinkled(5 * T + 1, 0.2, 5), what="5 tiles and a byte")


@pytest.mark.parametrize("tiles", ss.RANGE_SEAMS, ids=["G", "G + 1", "2 G + 1"])
def test_range_seams_of_the_whole_grid(tiles):
    # (one, two and three tiles a range; every range keeps an odd number of bases)
    text = ss.odd_ranges(tiles, G, seed=tiles)
    data, n = sg.want_of(text)
    packed, n_bases = pdev.seq_pack(sg.to_device(text))
    assert n_bases == n == tiles * T - len(range(0, tiles, -(-tiles // G)))
    assert packed.cpu().numpy().tobytes() == data


def test_bad_bytes_in_two_tiles_and_in_two_ranges(monkeypatch):
    text = ss.bases(6 * T, 21)
    text[3 * T + 5] = ord("n")  # the later one first in memory order of discovery or not: the smaller offset is named
    text[T + 9] = ord("N")
    for grid in (None, 1, 2):  # a tile a range; both tiles in one range; in two ranges of three tiles
        if grid is not None:
            monkeypatch.setenv("FLATGFA_SEQ_GRID", str(grid))
        assert sg.pack_error(sg.to_device(text)) == (-7, sg.bad_byte_message(ord("N"), T + 9)), grid
        assert sg.export_error(text) == (-7, sg.bad_byte_message(ord("N"), T + 9)), grid
    text[T + 9] = ord("A")
    assert sg.pack_error(sg.to_device(text)) == (-7, sg.bad_byte_message(ord("n"), 3 * T + 5))


@pytest.mark.parametrize("in_offset", range(1, 16))
def test_a_text_off_16_byte_alignment(in_offset):
    # the tiles are those of the aligned vectors: the text begins inside its first tile and ends where it ends
    check_raw(ss.sprinkled(T + 100, 0.2, in_offset), in_offset=in_offset, out_offset=(5 * in_offset) % 16, what=in_offset)
    check_raw(ss.bases(in_offset, in_offset), in_offset=in_offset, what=("short", in_offset))  # less than a vector


@pytest.mark.parametrize("out_offset", range(16))
def test_a_destination_off_16_byte_alignment(out_offset):
    check_raw(ss.sprinkled(2 * T + 77, 0.1, out_offset), out_offset=out_offset, what=out_offset)
    check_raw(ss.bases(2 * out_offset + 1, out_offset), out_offset=out_offset, what=("short", out_offset))


@pytest.mark.parametrize("carry", [0, 1, 2, 3])
def test_the_carry_goes_in_front(carry, monkeypatch):
    for name, text in ss.CHUNK_TEXTS.items():
        check_raw(text, carry=carry, what=(name, carry))
    check_raw(b"", carry=carry)  # a carry alone: one byte, the high nibble 0
    check_raw(ss.spaces(2 * T, 1), carry=carry)
    # the first range keeps nothing: the carry's high nibble is a later range's first base, which that range skips
    check_raw(ss.cat(ss.spaces(2 * T + 3, 2), ss.bases(T + 2, 3)), carry=carry, out_offset=carry + 1)
    monkeypatch.setenv("FLATGFA_SEQ_GRID", "2")
    check_raw(ss.cat(ss.spaces(2 * T + 3, 2), ss.bases(3 * T + 2, 3)), carry=carry)
    check_raw(ss.odd_ranges(4, 2, seed=carry), carry=carry)
    with pytest.raises(AssertionError):
        raw_pack(sg.to_device(b"ACGT"), carry=4)
    assert "carry" in _lib.last_error()


def test_a_stream_of_the_callers():
    import torch
    st = torch.cuda.Stream()
    text = ss.sprinkled(3 * T + 11, 0.25, 77)
    data, n = sg.want_of(text)
    packed, n_bases = pdev.seq_pack(sg.to_device(text), stream=st)
    letters = pdev.seq_unpack(packed, n_bases, stream=st)
    st.synchronize()  # (that stream only)
    assert n_bases == n and packed.cpu().numpy().tobytes() == data
    assert letters.cpu().numpy().tobytes() == sm.import_(sm.header(n) + data)


@pytest.mark.parametrize("offset", [0, 1, 8, 15])
def test_unpack_off_16_byte_alignment(offset):
    import torch
    n = 2 * T + 37
    seq = ss.bases(n, offset)
    data = sm.pack_codes(sm.codes_of(seq))
    room = torch.full((len(data) + 32,), 0xFF, dtype=torch.uint8, device="cuda:0")
    room[offset:offset + len(data)] = torch.from_numpy(data).to("cuda:0")
    out = torch.full((n + 64,), 0x55, dtype=torch.uint8, device="cuda:0")
    for out_offset in (0, 3, 16 - offset):
        out.fill_(0x55)
        rc = _lib.lib().flatgfa_dev_seq_unpack(room.data_ptr() + offset, n, out.data_ptr() + 16 + out_offset, None)
        assert rc == 0, _lib.last_error()
        got = out.cpu().numpy()
        at = 16 + out_offset
        assert got[at:at + n].tobytes() == seq.tobytes()
        assert (got[:at] == 0x55).all() and (got[at + n:] == 0x55).all()


# ---- past 2^32: device entries only, nothing of that size crosses to the host ----
PATTERN = b"ACTGGAT"  # (7 letters: 2^32 is no multiple of it, so an index that wraps shows)
WHITE = (5, 100, 1000)  # an odd number of whitespace bytes, all inside the first tile: base i is byte i + 3 from there on
BIG = (1 << 32) + 3 * T + 1


def big_window_codes(lo, hi):
    """The codes of bases [lo, hi), lo past the whitespace."""
    assert lo > WHITE[-1]
    i = np.arange(lo, hi, dtype=np.int64) + len(WHITE)
    return sm.codes_of(np.frombuffer(PATTERN, np.uint8)[i % len(PATTERN)])


def test_offsets_past_2_to_the_32():
    import torch
    d = torch.device("cuda:0")
    pattern = torch.from_numpy(np.frombuffer(PATTERN, np.uint8).copy()).to(d)
    text = pattern.repeat(BIG // len(PATTERN) + 1)[:BIG]
    for at in WHITE:
        text[at] = ord("\n")
    packed, n_bases = pdev.seq_pack(text)
    assert n_bases == BIG - len(WHITE)
    assert packed.numel() == (n_bases + 1) // 2
    # the start, by the model itself; then windows of a few KB on both sides of output byte 2^31 and at the end, by the formula
    head = text[:2 * T].cpu().numpy()
    assert packed[:T - 2].cpu().numpy().tobytes() == sm.pack_codes(sm.codes_of(head)).tobytes()[:T - 2]
    for lo, hi in (((1 << 31) - 4096, (1 << 31) + 4096), (packed.numel() - 4096, packed.numel())):
        want = sm.pack_codes(big_window_codes(2 * lo, min(2 * hi, n_bases)))
        assert packed[lo:hi].cpu().numpy().tobytes() == want.tobytes(), (lo, hi)
    assert n_bases & 1 == 0 or int(packed[-1]) >> 4 == 0
    del text
    letters = pdev.seq_unpack(packed, n_bases)
    assert letters.numel() == n_bases
    kept = sm.unpack_codes(sm.pack_codes(sm.codes_of(head)), len(sm.codes_of(head)))
    assert letters[:T].cpu().numpy().tobytes() == kept[:T].tobytes()
    for lo, hi in (((1 << 32) - 4096, (1 << 32) + 4096), (n_bases - 4096, n_bases)):
        want = np.frombuffer(sm.LETTERS, np.uint8)[big_window_codes(lo, hi)]
        assert letters[lo:hi].cpu().numpy().tobytes() == want.tobytes(), (lo, hi)
