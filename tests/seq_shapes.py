"""The inputs the packed-sequence tests share: file images with each header the reader refuses or accepts, and texts laid out
against the pack kernels' geometry (tests/seq_model.py: TILE bytes a tile, the tiles dealt to at most GRID workgroups in equal
contiguous ranges).  No device here."""
import struct

import numpy as np

import seq_model as sm

T, G = sm.TILE, sm.GRID
KNOWN = bytes([0x12] + [0] * 7 + [3] + [0] * 7 + [3] + [0] * 7 + [0, 0x10, 0x32, 0x03])  # ACTGG\n, flatgfa/tests/test.t
EMPTY = bytes([0x12] + [0] * 7 + [0] * 16 + [1])


def hdr(magic=0x12, length=3, capacity=3, hne=0):
    return struct.pack("<QQQB", magic, length, capacity, hne)


REFUSED = {
    "empty": b"",
    "shorter than the header": KNOWN[:24],
    "wrong magic": hdr(magic=0x13) + KNOWN[25:],
    "magic in the high bytes": hdr(magic=0x12 | 1 << 56) + KNOWN[25:],
    "high_nibble_end 2": hdr(hne=2) + KNOWN[25:],
    "high_nibble_end 255": hdr(hne=255) + KNOWN[25:],
    "capacity below len": hdr(capacity=2) + KNOWN[25:],
    "data cut short": KNOWN[:27],
    "padding missing": hdr(capacity=5) + KNOWN[25:] + b"\0",
    "no data, odd": hdr(length=0, capacity=0, hne=0),
    "len past the file": hdr(length=1 << 62, capacity=1 << 62),
}
ACCEPTED = {
    "known": (KNOWN, b"ACTGG"),
    "padding present": (hdr(capacity=5) + KNOWN[25:] + b"\xff\xff", b"ACTGG"),
    "trailing bytes": (KNOWN + b"garbage", b"ACTGG"),
    "unused nibble 0xF": (KNOWN[:27] + b"\xf3", b"ACTGG"),
    "even": (hdr(hne=1) + KNOWN[25:], b"ACTGGA"),
    "empty": (EMPTY, b""),
    "empty with capacity": (hdr(length=0, capacity=2, hne=1) + b"\xff\xff", b""),
}

_LETTERS = np.frombuffer(sm.LETTERS, np.uint8)
_SPACES = np.frombuffer(sm.WHITESPACE, np.uint8)


def bases(n, seed=0) -> np.ndarray:
    return _LETTERS[np.random.default_rng(seed).integers(0, 4, n)]


def spaces(n, seed=0) -> np.ndarray:
    return _SPACES[np.random.default_rng(seed).integers(0, len(_SPACES), n)]


def cat(*parts) -> np.ndarray:
    return np.concatenate([np.frombuffer(p, np.uint8) if isinstance(p, bytes) else p for p in parts])


def sprinkled(n, fraction, seed) -> np.ndarray:
    """n bytes, about `fraction` of them whitespace."""
    rng = np.random.default_rng(seed)
    t = bases(n, seed + 1000)
    at = rng.random(n) < fraction
    t[at] = spaces(int(at.sum()), seed + 2000)
    return t


def odd_ranges(tiles, grid, seed=0) -> np.ndarray:
    """`tiles` full tiles in which every range of the grid keeps an odd number of bases: one whitespace byte somewhere in each
    range's first tile.  So every range but the first begins on a high nibble or ends on a low one."""
    per = -(-tiles // grid)
    t = bases(tiles * T, seed)
    rng = np.random.default_rng(seed + 1)
    for first in range(0, tiles, per):
        t[first * T + int(rng.integers(0, T))] = ord("\n")
    return t


# tile seams: name -> (text, the grid the test asks for, or None for the library's own)
TILE_SEAMS = {
    "tile 1 begins on a high nibble": lambda: (cat(bases(T - 1, 1), b"\n", bases(T, 2)), None),
    "... in a range of its own tile pair": lambda: (cat(bases(T - 1, 1), b"\n", bases(T, 2)), 1),
    "tile 1 is all whitespace": lambda: (cat(bases(T - 1, 3), b" ", spaces(T, 4), bases(T + 5, 5)), None),
    "... inside one range": lambda: (cat(bases(T - 1, 3), b" ", spaces(T, 4), bases(T + 5, 5)), 1),
    # grid 4, 12 tiles: three tiles a range; tile 0 odd, tiles 1..7 whitespace (the rest of range 0, all of range 1, some of 2)
    "whitespace over a whole range and more": lambda: (cat(bases(T - 1, 6), b"\t", spaces(7 * T, 7), bases(4 * T, 8)), 4),
    "... with one range a tile": lambda: (cat(bases(T - 1, 6), b"\t", spaces(7 * T, 7), bases(4 * T, 8)), None),
    "a pending nibble, then whitespace to the end": lambda: (cat(bases(3, 9), spaces(2 * T + 17, 10)), None),
    "... over several ranges' tiles": lambda: (cat(bases(T + 1, 9), spaces(6 * T + 17, 10)), 2),
    "whitespace, then one base at the very end": lambda: (cat(spaces(3 * T, 11), b"G"), None),
    "a tile short of one byte": lambda: (bases(2 * T - 1, 12), None),
    "a tile and one byte": lambda: (bases(T + 1, 13), None),
}

# range seams on a small grid (FLATGFA_SEQ_GRID): (tiles, grid)
SMALL_GRID = 8
RANGE_SEAMS_SMALL = [(SMALL_GRID - 3, SMALL_GRID), (SMALL_GRID, SMALL_GRID), (SMALL_GRID + 1, SMALL_GRID), (2 * SMALL_GRID + 1, SMALL_GRID),
                     (3 * SMALL_GRID - 1, SMALL_GRID)]
# ... and on the library's own
RANGE_SEAMS = [G, G + 1, 2 * G + 1]

# host chunks: texts whose chunks keep odd counts, keep nothing, or are whitespace around a pending nibble
CHUNK_TEXTS = {
    "odd everywhere": b"A CT GGA\nTTC A\n",
    "whitespace around a pending nibble": b"ACG" + b" \n\t\r\x0c" * 5 + b"T" + b" " * 9 + b"GA \n",
    "only whitespace": b" \n" * 11,
    "one base": b"\n\nT\n\n",
    "no whitespace": bytes(bases(41, 14)),
    "sprinkled": bytes(sprinkled(150, 0.3, 15)),
}
CHUNKS = [1, 2, 3, 7, 4097]
