"""tests/seq_model.py against the format's known answers (the reference's own turnt input, flatgfa/tests/test.t), against its
second form, and against the header rules; and the geometry it mirrors against the source.  No device."""
import os
import struct

import numpy as np
import pytest

import seq_model as sm
from seq_shapes import ACCEPTED, EMPTY, KNOWN, REFUSED, hdr
from conftest import GOLDEN

SEQ = os.path.join(GOLDEN, "seq")


def read(name):
    with open(os.path.join(SEQ, name), "rb") as f:
        return f.read()


def test_geometry_is_the_sources():
    assert sm.source_constants() == {"TILE": sm.TILE, "THREADS": sm.THREADS, "GRID": sm.GRID}
    assert sm.TILE == 64 * sm.THREADS


def test_known_answer():
    assert read("test.txt") == b"ACTGG\n"
    assert len(KNOWN) == 28 and read("test.packed") == KNOWN
    assert sm.export(b"ACTGG\n") == KNOWN and sm.export_push(b"ACTGG\n") == KNOWN
    assert sm.import_(KNOWN) == b"ACTGG"
    assert sm.packed_info(KNOWN) == (5, 25)


@pytest.mark.parametrize("text", [b"", b" ", b"\n\n", b" \t\n\x0c\r"])
def test_empty_and_whitespace_only(text):
    assert len(EMPTY) == 25 and read("empty.packed") == EMPTY
    assert sm.export(text) == EMPTY and sm.export_push(text) == EMPTY
    assert sm.import_(EMPTY) == b"" and sm.packed_info(EMPTY) == (0, 25)


def test_round_trip_of_every_length_to_67():
    rng = np.random.default_rng(18)
    for n in range(68):
        seq = np.frombuffer(sm.LETTERS, np.uint8)[rng.integers(0, 4, n)].tobytes()
        file = sm.export(seq)
        assert file == sm.export_push(seq)
        assert len(file) == 25 + (n + 1) // 2 and file[24] == 1 - (n & 1)
        assert struct.unpack("<QQ", file[8:24]) == ((n + 1) // 2,) * 2
        if n & 1:
            assert file[-1] >> 4 == 0  # the unused high nibble
        assert sm.import_(file) == seq and sm.packed_info(file) == (n, 25)
        # whitespace anywhere changes nothing
        spaced = b" ".join(seq[i:i + 3] for i in range(0, n, 3)) + b"\r\n"
        assert sm.export(spaced) == file
        for chunk in (1, 2, 3, 7):
            assert sm.export_chunked(spaced, chunk) == file


def test_the_code_order_is_a_c_t_g():
    assert sm.export(b"ACTG")[25:] == bytes([0x10, 0x32])
    assert sm.export(b"GT")[25:] == bytes([0x23])


@pytest.mark.parametrize("bad", [b"a", b"N", b"\0", b"\xff", b"\x0b", b"*"])
def test_export_refuses(bad):
    text = b"ACGT \n" + bad + b"AC" + bad
    for f in (sm.export, sm.export_push):
        with pytest.raises(sm.SeqError) as e:
            f(text)
        assert e.value.offset == 6 and e.value.byte == bad[0]
        assert str(e.value) == f"seq-export: byte 0x{bad[0]:02x} at offset 6 is not a nucleotide"
    with pytest.raises(sm.SeqError) as e:
        sm.export_chunked(text, 4)
    assert e.value.offset == 6


@pytest.mark.parametrize("name", list(REFUSED))
def test_header_refusals(name):
    with pytest.raises(sm.SeqError):
        sm.packed_info(REFUSED[name])
    with pytest.raises(sm.SeqError):
        sm.import_(REFUSED[name])


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_header_acceptances(name):
    file, want = ACCEPTED[name]
    assert sm.import_(file) == want and sm.packed_info(file) == (len(want), 25)


def test_a_bad_nibble_names_the_first_base():
    file = hdr(length=3, capacity=3, hne=1) + bytes([0x10, 0x42, 0x34])
    with pytest.raises(sm.SeqError) as e:
        sm.import_(file)
    assert e.value.offset == 3 and e.value.byte == 4
    # ... but not in the unused nibble
    assert sm.import_(hdr(length=2, capacity=2, hne=0) + bytes([0x10, 0x42])) == b"ACT"


# ---- the shapes the GPU tests use are what their names say ----
def test_tile_seam_shapes():
    import seq_shapes as ss
    T = sm.TILE
    for name, make in ss.TILE_SEAMS.items():
        text, grid = make()
        assert text.dtype == np.uint8 and (grid is None or 1 <= grid <= sm.GRID), name
        assert sm.export(text) == sm.export_chunked(text.tobytes(), T), name  # (a chunk a tile: the carry is the tile's pending nibble)
    text, _ = ss.TILE_SEAMS["tile 1 begins on a high nibble"]()
    assert len(sm.codes_of(text[:T])) & 1
    text, _ = ss.TILE_SEAMS["whitespace over a whole range and more"]()
    assert len(sm.codes_of(text[:T])) & 1 and len(sm.codes_of(text[T:8 * T])) == 0 and len(text) == 12 * T
    text, _ = ss.TILE_SEAMS["a pending nibble, then whitespace to the end"]()
    assert sm.export(text)[24] == 0 and sm.export(text)[-1] >> 4 == 0


def test_range_seam_shapes():
    import seq_shapes as ss
    T = sm.TILE
    for tiles, grid in ss.RANGE_SEAMS_SMALL:
        text = ss.odd_ranges(tiles, grid, seed=tiles)
        per = -(-tiles // grid)
        assert len(text) == tiles * T
        for first in range(0, tiles, per):
            assert len(sm.codes_of(text[first * T:(first + per) * T])) & 1, (tiles, grid, first)
    assert ss.RANGE_SEAMS == [sm.GRID, sm.GRID + 1, 2 * sm.GRID + 1]


def test_chunk_texts_in_the_model():
    import seq_shapes as ss
    for name, text in ss.CHUNK_TEXTS.items():
        for chunk in ss.CHUNKS:
            assert sm.export_chunked(text, chunk) == sm.export(text) == sm.export_push(text), (name, chunk)
