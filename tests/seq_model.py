"""The packed-sequence codec in plain numpy / Python: what `fgfa seq-export` and `fgfa seq-import` (flatgfa/src/packedseq.rs,
cli/cmds.rs:415-452) make of a text and of a file, stated without any device in mind.  The GPU tests hold the library against
this byte for byte.

A file is a 25-byte header without padding -- u64 magic 0x12, u64 len, u64 capacity, u8 high_nibble_end, little-endian -- then
`len` data bytes: base 2k in the low nibble of byte k, base 2k + 1 in the high one, A 0, C 1, T 2, G 3.

Also here: the device code's geometry (seq_device.hpp), held against the source text by tests/test_seq_model.py.
"""
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pollen_amd", "csrc")

HEADER = 25
MAGIC = 0x12
LETTERS = b"ACTG"
WHITESPACE = b" \t\n\x0c\r"  # Rust's u8::is_ascii_whitespace: not \x0b
# seq_device.hpp: a tile of text, a workgroup's lanes, the most workgroups, the chunk of the host routes
TILE, THREADS, GRID = 16384, 256, 1024
CHUNK = 64 << 20


def source_constants():
    with open(os.path.join(CSRC, "seq_device.hpp")) as f:
        text = f.read()

    def one(pattern):
        (m,) = re.findall(pattern, text)
        return int(m)
    return {"TILE": one(r"constexpr uint32_t kSeqTile = (\d+);"), "THREADS": one(r"constexpr int kSeqThreads = (\d+);"),
            "GRID": one(r"constexpr uint32_t kSeqGrid = (\d+);")}


class SeqError(ValueError):
    """What the reference panics on.  offset: the text offset (export) or base index (a bad nibble), else None."""

    def __init__(self, msg, offset=None, byte=None):
        super().__init__(msg)
        self.offset, self.byte = offset, byte


_CODE = np.full(256, 0xFF, np.uint8)  # 0xFF: not a nucleotide; 0xFE: whitespace
for _i, _c in enumerate(LETTERS):
    _CODE[_c] = _i
for _c in WHITESPACE:
    _CODE[_c] = 0xFE


def codes_of(text) -> np.ndarray:
    """The codes of the kept bases of a text, in order; SeqError at the smallest offset of a byte that is neither."""
    t = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    c = _CODE[t]
    bad = np.flatnonzero(c == 0xFF)
    if len(bad):
        at = int(bad[0])
        raise SeqError(f"seq-export: byte 0x{int(t[at]):02x} at offset {at} is not a nucleotide", at, int(t[at]))
    return c[c != 0xFE]


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """Two codes a byte, the even one low; the unused last high nibble 0."""
    n = len(codes)
    even = np.zeros((n + 1) // 2 * 2, np.uint8)
    even[:n] = codes
    return (even[0::2] | (even[1::2] << 4)).astype(np.uint8)


def header(n_bases: int, capacity=None) -> bytes:
    length = (n_bases + 1) // 2
    return struct.pack("<QQQB", MAGIC, length, length if capacity is None else capacity, 0 if n_bases & 1 else 1)


def export(text) -> bytes:
    """The file image `fgfa seq-export` writes for a text."""
    codes = codes_of(text)
    return header(len(codes)) + pack_codes(codes).tobytes()


def export_push(text: bytes) -> bytes:
    """The same, the way the reference's writer does it: one push a nucleotide."""
    data, high_nibble_end = bytearray(), True
    for at, b in enumerate(text):
        if b in WHITESPACE:
            continue
        if b not in LETTERS:
            raise SeqError(f"seq-export: byte 0x{b:02x} at offset {at} is not a nucleotide", at, b)
        if high_nibble_end:
            data.append(LETTERS.index(b))
        else:
            data[-1] |= LETTERS.index(b) << 4
        high_nibble_end = not high_nibble_end
    return struct.pack("<QQQB", MAGIC, len(data), len(data), 1 if high_nibble_end else 0) + bytes(data)


def packed_info(file: bytes):
    """(n_bases, data_offset) of a file image, or SeqError for each header the reference's reader panics on."""
    if len(file) < HEADER:
        raise SeqError("the file is shorter than the header")
    magic, length, capacity, hne = struct.unpack("<QQQB", file[:HEADER])
    if magic != MAGIC:
        raise SeqError("wrong magic")
    if hne > 1:
        raise SeqError("high_nibble_end is not 0 or 1")
    if capacity < length:
        raise SeqError("capacity < len")
    if len(file) - HEADER < capacity:
        raise SeqError("fewer than capacity bytes behind the header")
    if length == 0 and hne == 0:
        raise SeqError("no data and an odd length")
    return 2 * length - (1 - hne), HEADER


def unpack_codes(data: np.ndarray, n_bases: int) -> np.ndarray:
    """The first n_bases nibbles as letters; SeqError at the smallest base index whose nibble is above 3."""
    nib = np.empty(2 * len(data), np.uint8)
    nib[0::2] = data & 0xF
    nib[1::2] = data >> 4
    nib = nib[:n_bases]
    bad = np.flatnonzero(nib > 3)
    if len(bad):
        at = int(bad[0])
        raise SeqError(f"seq-import: nibble {int(nib[at])} at base {at} is not a nucleotide", at, int(nib[at]))
    return np.frombuffer(LETTERS, np.uint8)[nib]


def import_(file: bytes) -> bytes:
    """The bases of a file image (`fgfa seq-import` prints them and one newline)."""
    n_bases, off = packed_info(file)
    data = np.frombuffer(file, np.uint8)[off:off + (n_bases + 1) // 2]
    return unpack_codes(data, n_bases).tobytes()


def export_chunked(text: bytes, chunk: int) -> bytes:
    """The host route's way through a text cut every `chunk` bytes: a chunk whose bases, with the carry in front of them, are
    an odd number keeps its last byte back unless it is the last chunk, and that byte's low nibble is the next chunk's carry."""
    out, carry, bases = bytearray(), None, 0
    for a in range(0, len(text), chunk):
        piece = text[a:a + chunk]
        try:
            codes = codes_of(piece)
        except SeqError as e:
            raise SeqError(f"seq-export: byte 0x{e.byte:02x} at offset {a + e.offset} is not a nucleotide", a + e.offset, e.byte)
        bases += len(codes)
        logical = codes if carry is None else np.concatenate([np.array([carry], np.uint8), codes])
        packed = pack_codes(logical)
        if a + chunk < len(text) and len(logical) & 1:
            carry = int(packed[-1]) & 0xF
            out += packed[:-1].tobytes()
        else:
            carry = None
            out += packed.tobytes()
    return header(bases) + bytes(out)
