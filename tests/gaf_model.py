"""A plain-Python restatement of the reference's pangenotype matrix, for the tests only.

cucapra/pollen flatgfa/src/ops/pangenotype.rs:11-70 (make_pangenotype_matrix) and flatgfa/src/namemap.rs:7-43 (NameMap),
rule by rule; the product (pollen_amd/) never imports it.  row() is slow -- a byte at a time -- and meant for small inputs;
row_fast() reads a line at a time, for texts of many MB, and tests/test_pangenotype_model.py pins it to row().
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence, Tuple

U64 = (1 << 64) - 1
TAB, NL, HASH, GT, LT = 9, 10, ord("#"), ord(">"), ord("<")


class GafError(Exception):
    """Where the reference panics: a name the graph does not have (namemap.rs:31, the HashMap index) or an id past the
    row (pangenotype.rs:60, name 0)."""

    def __init__(self, file: int, offset: int):
        super().__init__(f"GAF file {file}: the line at byte offset {offset} names a segment that is not in the graph")
        self.file = file
        self.offset = offset


def name_map(seg_names: Sequence[int]) -> Tuple[int, Dict[int, int]]:
    """NameMap::build (namemap.rs:36-42) over the segments' names in id order: (sequential_max, others)."""
    seq_max, others = 0, {}
    for i, name in enumerate(seg_names):
        nm1 = (int(name) - 1) & U64  # namemap.rs:20: `name - 1` wraps in a release build
        if nm1 == seq_max and nm1 == i:
            seq_max += 1  # namemap.rs:21
        else:
            others[int(name)] = i  # namemap.rs:23 (a later duplicate replaces an earlier one)
    return seq_max, others


def lookup(nm: Tuple[int, Dict[int, int]], num: int):
    """NameMap::get (namemap.rs:27-33), or None where it panics on a missing key."""
    seq_max, others = nm
    if num <= seq_max:
        return ((num - 1) & U64) & 0xFFFFFFFF  # namemap.rs:29: `(name - 1) as u32`
    return others.get(num)


def row(text: bytes, seg_names: Sequence[int], file: int = 0, nm=None) -> List[bool]:
    """One row of the matrix: the body of the loop over files (pangenotype.rs:18-66)."""
    nm = nm if nm is not None else name_map(seg_names)
    S = len(seg_names)
    out = [False] * S
    start = 0
    while True:
        pos = text.find(b"\n", start)  # pangenotype.rs:22: memchr; bytes after the last '\n' are never a line
        if pos < 0:
            break
        line, line_off = text[start:pos], start
        start = pos + 1  # pangenotype.rs:25
        if not line or line[0] == HASH:  # pangenotype.rs:27-29
            continue
        tab_count, idx = 0, 0
        while idx < len(line) and tab_count < 5:  # pangenotype.rs:31-38
            if line[idx] == TAB:
                tab_count += 1
            idx += 1
        if tab_count < 5 or idx >= len(line):  # pangenotype.rs:40-42
            continue
        end_idx = idx
        while end_idx < len(line) and line[end_idx] != TAB:  # pangenotype.rs:44-47
            end_idx += 1
        field = line[idx:end_idx]
        p = 0
        while p < len(field):  # pangenotype.rs:51-64
            b = field[p]
            if b == GT or b == LT:
                p += 1
                num = 0
                while p < len(field) and 48 <= field[p] <= 57:  # is_ascii_digit
                    num = (num * 10 + (field[p] - 48)) & U64  # usize arithmetic wraps in a release build
                    p += 1
                sid = lookup(nm, num)
                if sid is None or sid >= S:  # the HashMap index panics / matrix[file_idx][..] is out of bounds
                    raise GafError(file, line_off)
                out[sid] = True
            else:
                p += 1
    return out


def matrix(texts: Sequence[bytes], seg_names: Sequence[int]) -> List[List[bool]]:
    """make_pangenotype_matrix over GAF texts (pangenotype.rs:11-70), one row per text."""
    nm = name_map(seg_names)
    return [row(t, seg_names, f, nm) for f, t in enumerate(texts)]


def table(texts: Sequence[bytes], seg_names: Sequence[int]) -> bytes:
    """What `fgfa matrix GAF` prints (cmds.rs:465-474)."""
    return b"".join(b"".join(b"1" if c else b"0" for c in r) + b"\n" for r in matrix(texts, seg_names))


# ---- the same rules a line at a time, for texts of many MB ----

_TOKEN = re.compile(rb"[<>]([0-9]*)")
_FOLD = 19  # decimal digits that always fit in a u64


def digits_mod_2_64(digits: bytes) -> int:
    """The u64 that wrapping `num * 10 + d` reads from a run of ASCII digits (pangenotype.rs:55-58).  Python's int() refuses
    strings of more than sys.get_int_max_str_digits() digits, so the run is folded 19 digits at a time."""
    digits = digits.lstrip(b"0")
    v = 0
    for i in range(0, len(digits), _FOLD):
        part = digits[i:i + _FOLD]
        v = (v * 10 ** len(part) + int(part)) & U64
    return v


def row_fast(text: bytes, seg_names: Sequence[int], file: int = 0, nm=None) -> List[bool]:
    """What row() gives, line by line: split at '\\n' (the tail behind the last one is no line), skip empty and '#' lines,
    the path field is the 6th tab-separated part, every '>' or '<' in it starts a token."""
    nm = nm if nm is not None else name_map(seg_names)
    S = len(seg_names)
    out = [False] * S
    off = 0
    for line in text[:text.rfind(b"\n") + 1].split(b"\n")[:-1]:
        line_off, off = off, off + len(line) + 1
        if not line or line[0] == HASH:
            continue
        parts = line.split(b"\t", 6)
        if len(parts) < 6:
            continue
        for digits in set(_TOKEN.findall(parts[5])):
            sid = lookup(nm, digits_mod_2_64(digits))
            if sid is None or sid >= S:
                raise GafError(file, line_off)
            out[sid] = True
    return out


def matrix_fast(texts: Sequence[bytes], seg_names: Sequence[int]) -> List[List[bool]]:
    """matrix() by row_fast."""
    nm = name_map(seg_names)
    return [row_fast(t, seg_names, f, nm) for f, t in enumerate(texts)]
