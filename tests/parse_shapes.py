"""Texts for the tests of the device GFA parser, and the plain grammar restated in Python.

`reason(text, stream)` says, from the grammar of DESIGN.md section 20 alone -- one regular expression per line kind, never
the library's answer -- which route a text takes: "plain" (the device makes the pools) or why the host parser judges it
("grammar", "limit", "name": the first of these that holds anywhere in the text).  `plain` is `reason(...) == "plain"`.

The builders take the tile size T the library reports (flatgfa_parse_device_info) and lay an item, a field end or a
newline on a tile edge; each asserts from the text alone that it does."""
import glob
import os
import re

import numpy as np

from oracle import flatgfa_oracle as fo
from print_shapes import (HANDMADE, TAIL, bases, digit_names, long_cigar, long_optional, long_overlaps, one_long_segment,  # noqa: F401
                          path_name, s_block, with_pools)



def all_golden_gfas() -> list:
    """Every GFA text under tests/golden: the thirteen at the top (conftest.golden_gfas) and the inputs and expected outputs
    of chop, crush, flatten, the GAF lookup, inject and the sequence codec below it."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return sorted(glob.glob(os.path.join(root, "**", "*.gfa"), recursive=True))


def golden_id(path: str) -> str:
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return os.path.relpath(path, root)[:-4]


WINDOW = 32          # parse_device.hpp: kParseWindow, the digits of one number the kernels read
SCAN_TILE = 256 * 4  # parse_device.hpp: kParseScanTile, the elements of one tile of the scans the parser runs

# the texts tests/test_host.py adds to its QUIRKS inside a decorator
ADDED = [
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+,2+,\t*\n",      # a trailing comma is accepted
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,,1+\t*\n",         # an empty item is not
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+,3+,1+\t*\n",    # unknown segment in a later chunk
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+2+\t*\n",        # a missing comma
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,+,1+\t*\n",        # a sign without a name
    b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+,2+\t*\nL\t1\t+\t2\t+\t0M\nP\tq\t2+,2+,1-\t1M,2M\n",
]
# The QUIRKS of tests/test_host.py the grammar excludes, by index, with the reason; every other entry is plain.
QUIRKS_NOT_PLAIN = {
    3: "grammar",   # an empty line
    4: "name",      # a step names no segment
    5: "grammar",   # a garbage byte behind the last step
    6: "grammar",   # two of them
    7: "grammar",   # a name without a sign ends the field
    8: "grammar",   # a sign without digits
    13: "grammar",  # another line kind
    14: "grammar",  # no tab at byte 1
    15: "grammar",  # a name that is no number
    16: "grammar",  # no tab behind the name
    17: "grammar",  # a second header
    18: "grammar",  # ... which the host parser accepts behind an empty one
    20: "grammar",  # no overlaps column
    21: "grammar",  # a tab inside the step field
    23: "grammar",  # an op longer than 255
    24: "grammar",  # digits without an op letter
    25: "name",     # a link names no segment
    26: "grammar",  # a tab inside the CIGAR
    27: "grammar",  # '*' as one of several overlaps
    29: "grammar",  # "*\r" is no overlaps field
}
ADDED_NOT_PLAIN = {0: "grammar", 1: "grammar", 2: "name", 3: "grammar", 4: "grammar"}

_CIGAR = rb"(?:[0-9]+[MNDI])+"
_H = re.compile(rb"H\t.*", re.S)
_S = re.compile(rb"S\t([0-9]+)\t[^\t]*(?:\t.*)?", re.S)
_L = re.compile(rb"L\t([0-9]+)\t[+-]\t([0-9]+)\t[+-]\t((?:[0-9]+[MNDI])*)", re.S)
_P = re.compile(rb"P\t[^\t]*\t((?:[0-9]+[+-](?:,[0-9]+[+-])*)?)\t(\*|" + _CIGAR + rb"(?:," + _CIGAR + rb")*)", re.S)
_OP = re.compile(rb"([0-9]+)[MNDI]")
_ITEM = re.compile(rb"([0-9]+)[+-]")


def lines_of(text: bytes, stream: bool) -> list:
    """parse_mem drops what follows the last newline; parse_stream keeps an unterminated last line."""
    parts = text.split(b"\n")
    last = parts.pop()
    if stream and last:
        parts.append(last)
    return parts


def reason(text: bytes, stream: bool = False) -> str:
    headers, long_number, seg_names, used = 0, False, set(), []

    def number(digits: bytes) -> int:
        nonlocal long_number
        long_number |= len(digits) > WINDOW
        return int(digits) % (1 << 64)

    def ops_fit(field: bytes) -> bool:
        nonlocal long_number
        for m in _OP.finditer(field):
            if len(m.group(1)) > WINDOW:
                long_number = True
            elif int(m.group(1)) % (1 << 32) > 255:
                return False
        return True

    for line in lines_of(text, stream):
        kind = line[:1]
        if kind == b"H" and _H.fullmatch(line):
            headers += 1
            if headers > 1:
                return "grammar"
        elif kind == b"S" and (m := _S.fullmatch(line)):
            seg_names.add(number(m.group(1)))
        elif kind == b"L" and (m := _L.fullmatch(line)):
            used += [number(m.group(1)), number(m.group(2))]
            if not ops_fit(m.group(3)):
                return "grammar"
        elif kind == b"P" and (m := _P.fullmatch(line)):
            used += [number(d) for d in _ITEM.findall(m.group(1))]
            if not ops_fit(m.group(2)):
                return "grammar"
        else:
            return "grammar"
    if long_number:
        return "limit"
    # NameMap::get (namemap.rs:27-33): name 0 is "sequential" and wraps to no segment, whatever the segments are called
    if any(n == 0 or n not in seg_names for n in used):
        return "name"
    return "plain"


def plain(text: bytes, stream: bool = False) -> bool:
    return reason(text, stream) == "plain"


def pools_of(g) -> dict:
    return {name: g.pool(name).tobytes() for name in fo.POOL_ORDER}


def normalized_pools(g) -> dict:
    """A handle's pools as its text in normalized order (print.rs:134-150) gives them back: no line order, and the alignment
    pool laid out as that text lists it -- every path's overlaps, then every link's -- with an empty alignment as the `0M`
    the printer writes for it (print.rs:26-31; chop and inject make links with such overlaps).  For a graph parsed from a
    text in that order this changes the line order alone."""
    p = {name: g.pool(name).copy() for name in fo.POOL_ORDER}
    al, ovl, links = p["alignment"], p["overlaps"].copy(), p["links"].copy()
    out = []

    def moved(start, end):
        ops = al[start:end].tolist() or [0]  # 0M
        out.extend(ops)
        return len(out) - len(ops), len(out)

    for path in p["paths"]:
        for k in range(int(path["ov_start"]), int(path["ov_end"])):
            ovl[k] = moved(int(ovl[k]["start"]), int(ovl[k]["end"]))
    for k in range(len(links)):
        links[k]["ov_start"], links[k]["ov_end"] = moved(int(links[k]["ov_start"]), int(links[k]["ov_end"]))
    p.update(alignment=np.array(out, dtype=al.dtype), overlaps=ovl, links=links, line_order=p["line_order"][:0])
    return {name: a.tobytes() for name, a in p.items()}


# ---- steps on tile edges ----

def steps_exact(n: int, a: int = 1, b: int = 10) -> bytes:
    """A step field of exactly n >= 2 bytes over the one-digit name a and the two-digit name b, both orientations."""
    k, extra = (n + 1) // 3, (n + 1) % 3  # k items of "a+" and commas are 3k - 1 bytes; a two-digit name adds one
    assert k >= extra
    items = [b"%d%s" % (b if i < extra else a, b"+-"[i % 2:i % 2 + 1]) for i in range(k)]
    out = b",".join(items)
    assert len(out) == n, (n, len(out))
    return out


def item_on_edge(T: int, k: int) -> bytes:
    """The item `12345+,` laid so that byte T of the text is its byte k (k = -1: the byte before it, 7: the one behind)."""
    head, front = b"S\t12345\tACGT\n", b"P\tp\t1+,"
    pad = s_block(T - k - len(head) - len(front))[0]
    text = head + pad + front + b"12345+,1-\t*\n"
    assert text.index(b"12345+,") + k == T
    return text


def field_begins_on_tile(T: int) -> bytes:
    front = b"P\tp\t"
    text = s_block(T - len(front))[0] + front + b"1+,2-,3+\t*\n"
    assert text.index(b"1+,2-") == T
    return text


def field_ends_on_tile(T: int) -> bytes:
    """A step field whose last byte is the last byte of the text's second tile."""
    head = s_block(T - 100)[0] + b"P\tp\t"
    text = head + steps_exact(2 * T - len(head)) + b"\t*\nP\tq\t2+\t*\n"
    assert text.index(b"\t*\n") == 2 * T
    return text


def short_lines_in_one_tile(T: int) -> bytes:
    """Five whole P lines inside the second tile, one of them without steps, one of one step."""
    text = s_block(T + 40)[0] + b"P\ta\t1+,2-\t*\nP\tempty\t\t*\nP\tb\t3-\t2M\nP\tc\t1+,1+,1-\t1M,2M\nP\td\t2+\t*\n" + s_block(T, 500)[0]
    assert T < text.index(b"P\ta") and text.index(b"P\td\t2+\t*\n") + 9 < 2 * T
    return text


def line_across_tiles(T: int) -> bytes:
    """One P line that starts in the first tile and ends in the fourth."""
    text = s_block(T // 2)[0] + b"P\tlong\t" + steps_exact(3 * T) + b"\t*\nP\tafter\t1-\t*\n"
    assert text.index(b"\t*\n") // T - text.index(b"P\tlong") // T >= 3
    return text


def many_short_paths(n: int = 1000) -> bytes:
    out = [b"S\t%d\tA" % i for i in range(1, 8)]
    for i in range(n):
        out.append(b"P\tp%d\t" % i + b",".join(b"%d%s" % (1 + (i + j) % 7, b"+-"[(i * j) % 2:(i * j) % 2 + 1]) for j in range(1 + i % 5)) + b"\t*")
    return b"\n".join(out) + b"\n"


def newline_ends_tile(T: int) -> bytes:
    text = s_block(T)[0] + TAIL
    assert text[T - 1:T] == b"\n" and text[T:T + 1] != b"\n"
    return text


def newline_begins_tile(T: int) -> bytes:
    text = s_block(T + 1)[0] + TAIL
    assert text[T:T + 1] == b"\n"
    return text


# ---- names ----

def reversed_names(n: int = 300) -> bytes:
    out = [b"S\t%d\tAC" % i for i in range(n, 0, -1)]
    out.append(b"P\tp\t" + b",".join(b"%d%s" % (i, b"+-"[i % 2:i % 2 + 1]) for i in range(1, n + 1)) + b"\t*")
    out.append(b"L\t1\t+\t%d\t-\t0M" % n)
    return b"\n".join(out) + b"\n"


def skipped_names(n: int = 3000) -> bytes:
    """Every second name: all but none are outside the sequential prefix, a table of n names searched by bisection."""
    names = list(range(2, 2 * n + 2, 2))
    out = [b"S\t%d\tG" % i for i in names]
    out.append(b"P\tp\t" + b",".join(b"%d%s" % (i, b"+-"[(i // 2) % 2:(i // 2) % 2 + 1]) for i in names[::3]) + b"\t*")
    out.append(b"L\t%d\t+\t%d\t+\t1M" % (names[0], names[-1]))
    return b"\n".join(out) + b"\n"


def duplicate_names(T: int, sequential: bool) -> bytes:
    """The two duplicate-name quirks of tests/test_host.py grown past a tile: names 1..n twice over (the first id wins), or
    names 5, 5, 7, 7, ... (the later id wins)."""
    n = T // 6 + 10
    names = list(range(1, n + 1)) * 2 if sequential else [5 + 2 * (i // 2) for i in range(2 * n)]
    out = [b"S\t%d\t%s" % (name, b"ACGT"[i % 4:i % 4 + 1]) for i, name in enumerate(names)]
    out.append(b"P\tp\t" + b",".join(b"%d+" % name for name in names[::5]) + b"\t*")
    text = b"\n".join(out) + b"\n"
    assert len(text) > T
    return text


# ---- the scans' spine ----

def scan_spine(T: int) -> bytes:
    """More text tiles than one tile of the tiled scan holds: paths longer than a tile, paths shorter than a lane's 16
    bytes, both orientations."""
    rng = np.random.default_rng(5)
    n_segs = 900
    out = [b"S\t%d\tA" % i for i in range(1, n_segs + 1)]
    size, want = 0, (SCAN_TILE + 3) * T
    names = [b"%d" % i for i in range(1, n_segs + 1)]
    k = 0
    while size < want:
        for n_steps in (T, 1, 2, 3 * T // 2):
            ids = rng.integers(0, n_segs, n_steps)
            signs = rng.integers(0, 2, n_steps)
            line = b"P\t%d\t" % k + b",".join(names[i] + (b"+", b"-")[s] for i, s in zip(ids.tolist(), signs.tolist())) + b"\t*"
            out.append(line)
            size += len(line) + 1
            k += 1
    text = b"\n".join(out) + b"\n"
    assert len(text) > SCAN_TILE * T
    return text


# ---- the verdict at lane, tile and wave seams (tests/test_gpu_parse_seams.py) ----

LANE = 16  # parse_device.hpp: kParseLaneBytes, the text bytes of one lane of the step kernels
WAVE = 64  # the bytes wave_cigar, wave_find_tab, wave_find_last_tab and wave_copy take a step
ZEROS = b"0" * 32


def on_edge(T: int, x: int, k: int, item: bytes, tail: bytes = b"1-\t*\n") -> bytes:
    """`item` inside the step field of a P line, laid so that byte x of the text (a lane's first byte; a tile's, where x is a
    multiple of T) is the item's byte k (k = -1: the comma before it, len(item): the first byte of `tail`).  Segments 1, 2,
    ... and 12345 exist; `tail` ends the line."""
    head, front = b"S\t12345\tACGT\n", b"P\tp\t1+,"
    assert x % LANE == 0 and -1 <= k <= len(item)
    text = s_block(x - k - len(head) - len(front))[0] + head + front + item + tail
    at = x - k
    assert text[at:at + len(item)] == item and text[at - len(front):at] == front and text.endswith(b"\n")
    assert (text[x:x + 1] == item[k:k + 1]) if 0 <= k < len(item) else (text[x:x + 1] == (b"," if k < 0 else tail[:1]))
    return text


# item -> (reason, what the host parser does with the text): laid inside a step field, in front of "1-\t*\n".  The class
# holds wherever the item lies (tests/test_parse_shapes.py asserts it for every k).
STEP_ITEMS = {
    b"12345+,": ("plain", "accepts"),
    b"0" * 27 + b"12345+,": ("plain", "accepts"),   # 32 digits: the window
    b"0" * 28 + b"12345+,": ("limit", "accepts"),   # 33
    b"1+,,": ("grammar", "error"),                  # an empty item
    b"1+2+,": ("grammar", "error"),                 # a missing comma
    b"12345,": ("grammar", "error"),                # a name without a sign
    b"1+,+,": ("grammar", "error"),                 # a sign without a name
    b"1+x,": ("grammar", "error"),
    b"1+\t1+,": ("grammar", "error"),               # a tab inside the field
    b"1+\r,": ("grammar", "error"),
    b"1+*,": ("grammar", "error"),
    b"99999+,": ("name", "error"),
    b"0+,": ("name", "error"),
}
# ... and items that end the step field and the line themselves, in front of the line "P\tq\t1-\t*\n": the field's end, the tab
# before the overlaps and the overlaps column move over the edge.  "grammar" with "accepts" is where the device must stand
# aside and the host parser's handle come back.
FIELD_END_TAIL = b"P\tq\t1-\t*\n"
FIELD_ENDS = {
    b"1+,\t*\n": ("grammar", "accepts"),            # a trailing comma
    b"1+,12345\t*\n": ("grammar", "accepts"),       # a name without a sign ends the field
    b"1+,1+x\t*\n": ("grammar", "accepts"),         # a swallowed garbage byte
    b"1+,1+xy\t*\n": ("grammar", "error"),          # two of them
    b"1+\t\n": ("grammar", "accepts"),              # an empty overlaps column
    b"1+\t1M,\n": ("grammar", "accepts"),
    b"1+\t1M,*\n": ("grammar", "error"),
    b"1+\t256M\n": ("grammar", "error"),
    b"1+\tM\n": ("grammar", "error"),
    b"1+\t*\r\n": ("grammar", "error"),
    b"1+\n": ("grammar", "accepts"),                # no overlaps column
}


def outcome(text: bytes, stream: bool, parse) -> str:
    """"plain", "accepted" (not plain, and `parse` -- the host parser -- gives a handle) or "error"."""
    if plain(text, stream):
        return "plain"
    try:
        parse(text).close()
    except Exception:
        return "error"
    return "accepted"


# ---- CIGARs by the wave's 64-byte steps ----

def _op(i: int, size: int) -> bytes:
    """Op i of `size` bytes: one, two or three digits (at most 255) and one of the four letters."""
    value = (i % 10, 10 + (7 * i) % 90, 100 + (13 * i) % 156)[size - 2]
    return b"%d%c" % (value, b"MNDI"[i % 4])


def cigar_exact(n: int, commas: bool = False):
    """A valid CIGAR of exactly n bytes (an L line's: the empty one counts) or, with `commas`, a valid overlaps field (a P
    line's: '*' is the one of one byte); None where there is none.  Ops of one, two and three digits, all four letters."""
    if n == 0:
        return None if commas else b""
    if n == 1:
        return b"*" if commas else None
    out, left, i = [], n, 0
    while left:
        size = next(s for s in ((2, 3, 4)[(i + j) % 3] for j in range(3)) if left - s == 0 or left - s >= 2)
        out.append(_op(i, size))
        left -= size
        if commas and i % 3 == 1 and left >= 3:
            out.append(b",")
            left -= 1
        i += 1
    field = b"".join(out)
    assert len(field) == n and re.fullmatch(_CIGAR + rb"(?:," + _CIGAR + rb")*" if commas else _CIGAR, field), (n, field)
    return field


def cigar_text(field: bytes, commas: bool) -> bytes:
    """`field` as the CIGAR of an L line or, with `commas`, the overlaps of a P line."""
    line = b"P\tp\t1+,2-\t" + field + b"\n" if commas else b"L\t1\t+\t2\t-\t" + field + b"\n"
    text = b"S\t1\tAC\nS\t2\tG\n" + line + b"P\tafter\t2+\t*\n"
    assert text.split(b"\n")[2].split(b"\t")[-1] == field or b"\t" in field or b"\n" in field
    return text


CIGAR_LEN = 200
FAULT_AT = [0, 1, 62, 63, 64, 65, 127, 128, 129, 199]  # around the wave's steps: byte 0 of a step takes its predecessor from the step before
FAULT_EDITS = [b"x", b",", b"M", b"\t", b"9"]


def cigar_fault(j: int, edit: bytes, commas: bool) -> bytes:
    """A CIGAR (an overlaps field) of 200 bytes with byte j replaced by `edit`."""
    field = cigar_exact(CIGAR_LEN, commas)
    field = field[:j] + edit + field[j + 1:]
    assert len(field) == CIGAR_LEN and field[j:j + 1] == edit
    return cigar_text(field, commas)


def cigar_joined(left: int, middle: bytes, commas: bool) -> bytes:
    """A 200-byte field: a valid one of `left` bytes, `middle` from byte `left` on, a valid one behind it."""
    a, b = cigar_exact(left, commas), cigar_exact(CIGAR_LEN - left - len(middle), commas)
    field = a + middle + b
    assert len(field) == CIGAR_LEN and field[left:left + len(middle)] == middle and a[-1:] in b"MNDI" and b[:1].isdigit()
    return cigar_text(field, commas)


# id -> (bytes before the middle, the middle): numbers and op letters across byte 64 of the field, where the wave's second step
# begins; the walk back over an op's digits crosses it
CIGAR_STRADDLES = {
    "256M, the 2 at byte 63": (63, b"256M"),                       # grammar
    "255M, the 2 at byte 63": (63, b"255M"),                       # plain
    "256M, the M at byte 64": (61, b"256M"),
    "33 digits, 16 before byte 64": (48, b"0" * 30 + b"255M"),     # limit
    "32 digits, 16 before byte 64": (48, b"0" * 29 + b"255M"),     # plain
    "33 digits, the M at byte 64": (31, b"0" * 30 + b"255M"),
    "32 digits, the M at byte 64": (32, b"0" * 29 + b"255M"),
    "33 digits, one before byte 64": (63, b"0" * 30 + b"255M"),
    "33 digits, 16 before byte 128": (112, b"0" * 30 + b"255M"),
    "33 digits, the M at byte 128": (95, b"0" * 30 + b"255M"),
    "32 digits, the M at byte 128": (96, b"0" * 29 + b"255M"),
    "32 digits worth 256, 16 before byte 64": (48, b"0" * 29 + b"256M"),  # grammar
    "33 digits worth 256, 16 before byte 64": (48, b"0" * 30 + b"256M"),  # limit: the host parser's to judge
    "an op letter at byte 64 behind one": (64, b"M"),              # grammar
    "an op letter at byte 128 behind one": (128, b"N"),
    "a comma at byte 63, a letter at 64": (63, b",M"),
    "a comma at byte 64": (64, b","),                              # plain between CIGARs, grammar inside one
    "a comma at byte 128": (128, b","),
    "two commas, the second at byte 64": (63, b",,"),
}


def cigar_family() -> dict:
    """id -> text: every single edit and every straddle, as an L line's CIGAR and as a P line's overlaps."""
    out = {}
    for commas in (False, True):
        form = "P" if commas else "L"
        for j in FAULT_AT:
            for edit in FAULT_EDITS:
                out["%s: %r at byte %d" % (form, edit.decode(), j)] = cigar_fault(j, edit, commas)
        for name, (left, middle) in CIGAR_STRADDLES.items():
            out["%s: %s" % (form, name)] = cigar_joined(left, middle, commas)
    return out


# ---- field lengths on the wave's steps ----

LADDER = range(0, 131)
STRETCHES = [2, 3, 4, 5] + list(range(60, 71)) + list(range(124, 133))


def ladder_stretches() -> list:
    """(steps, overlaps) whose "<steps>\\t<overlaps>" -- what wave_find_last_tab searches from the line's end -- is of every
    length in STRETCHES, with the last tab at its first byte (no steps), as near its end as a plain line has it (the
    overlaps '*') and in between.  A stretch of one byte is an empty overlaps column, which is not plain (FIELD_ENDS)."""
    out = []
    for n in STRETCHES:
        out.append((b"", cigar_exact(n - 1, True)))
        if n - 2 != 1:
            out.append((steps_exact(n - 2) if n > 2 else b"", b"*"))
        s = (n - 1) // 2
        if s >= 2 and n - 1 - s >= 2:
            out.append((steps_exact(s), cigar_exact(n - 1 - s, True)))
    assert all(len(s) + 1 + len(o) in STRETCHES for s, o in out) and {len(s) + 1 + len(o) for s, o in out} == set(STRETCHES)
    return out


def field_ladder() -> bytes:
    """One plain text in which a sequence, the optional bytes, a path name, a CIGAR and an overlaps field take every length
    from 0 to 130 -- around one and two of the wave's 64-byte steps -- and a P line's steps and overlaps together every
    length of STRETCHES."""
    out, name = [], 0
    for i in LADDER:
        out.append(b"S\t%d\t%s\t%s" % (name + 1, bases(i, i), bases(130 - i, 200 + i).lower()))
        out.append(b"S\t%d\t%s" % (name + 2, bases(i, 400 + i)))
        name += 2
    for i in LADDER:
        out.append(b"P\t%s\t1+,10-\t*" % (b"name_of_a_path." * 9)[:i])
        if cigar_exact(i) is not None:
            out.append(b"L\t%d\t+\t%d\t-\t%s" % (1 + i, 2 + i, cigar_exact(i)))
        if cigar_exact(i, True) is not None:
            out.append(b"P\tov%d\t1+,2-\t%s" % (i, cigar_exact(i, True)))
    for k, (steps, ovl) in enumerate(ladder_stretches()):
        out.append(b"P\tst%d\t%s\t%s" % (k, steps, ovl))
    text = b"\n".join(out) + b"\n"
    lines = [ln.split(b"\t") for ln in out]
    want = set(LADDER)
    assert {(len(f[2]), len(f[3])) for f in lines if f[0] == b"S" and len(f) == 4} == {(i, 130 - i) for i in LADDER}
    assert {len(f[2]) for f in lines if f[0] == b"S" and len(f) == 3} == want
    assert {len(f[1]) for f in lines if f[0] == b"P"} >= want
    assert {len(f[5]) for f in lines if f[0] == b"L"} == want - {1}
    assert {len(f[3]) for f in lines if f[0] == b"P" and f[1].startswith(b"ov")} == want - {0}
    assert {len(f[2]) + 1 + len(f[3]) for f in lines if f[0] == b"P" and f[1].startswith(b"st")} == set(STRETCHES)
    return text


# ---- the line index and the text's end ----

LAST_LINE = b"P\tlast\t1+,2-\t*"


def line_index_texts(T: int) -> dict:
    """id -> text: what k_line_fill judges -- a kind byte, the tab behind it, an empty line, a second header -- on a tile edge."""
    out = {}
    for at in (T - 1, T):
        out["kind X at byte %s" % ("T" if at == T else "T - 1")] = text = s_block(at)[0] + b"X\t1\tA\n" + TAIL
        assert text[at:at + 1] == b"X"
    out["no tab at byte T"] = text = s_block(T - 1)[0] + b"S1\tA\n" + TAIL
    assert text[T - 1:T + 1] == b"S1" and text[T - 2:T - 1] == b"\n"
    out["an empty line across T"] = text = s_block(T)[0] + b"\n" + TAIL
    assert text[T - 1:T + 1] == b"\n\n"
    head = b"H\tVN:Z:1.0\n"
    out["a second header at T"] = text = head + s_block(T - len(head))[0] + b"H\tVN:Z:2.0\n" + TAIL
    assert text[T:T + 2] == b"H\t" and text[T - 1:T] == b"\n"
    out["the one header at T"] = text = s_block(T)[0] + b"H\tVN:Z:2.0\n" + TAIL  # (plain: the same line index, no fault)
    assert text[T:T + 2] == b"H\t"
    return out


def unterminated(T: int, r: int, fault: bool) -> bytes:
    """A text of T + 16 + r bytes whose last line has no newline: load16's scalar tail reads r bytes of it.  `fault`: its last
    byte is no overlaps field.  parse_mem never sees the line; parse_stream takes it."""
    text = s_block(T + LANE + r - len(LAST_LINE))[0] + (LAST_LINE[:-1] + b"x" if fault else LAST_LINE)
    assert len(text) == T + LANE + r and text[-len(LAST_LINE):-1] == LAST_LINE[:-1] and text[-len(LAST_LINE) - 1:-len(LAST_LINE)] == b"\n"
    return text


def lone_kind(T: int, kind: bytes) -> bytes:
    """The text's last byte is a kind byte at byte T: the tab behind it would be read past the text's end."""
    text = s_block(T)[0] + kind
    assert len(text) == T + 1 and text[T - 1:] == b"\n" + kind
    return text


# ---- the first of grammar, limit and name, whichever kernel and tile finds which ----

_LONG1 = ZEROS + b"1"  # 33 digits
FAULTS = {
    "grammar": {"kind byte": b"X\t1\tA\n", "S name": b"S\tabc\tA\n", "L orientation": b"L\t1\tx\t2\t+\t0M\n",
                "CIGAR byte": b"L\t1\t+\t2\t+\t1X\n", "step byte": b"P\tg\t1+,x\t*\n"},
    "limit": {"S name": b"S\t" + ZEROS[:26] + b"7777777\tA\n", "L name": b"L\t" + _LONG1 + b"\t+\t2\t+\t0M\n",
              "CIGAR": b"L\t1\t+\t2\t+\t" + _LONG1 + b"M\n", "step name": b"P\tl\t2-," + _LONG1 + b"+\t*\n"},
    "name": {"link": b"L\t8888888\t+\t2\t+\t0M\n", "step": b"P\tn\t1+,8888888+\t*\n"},
}
PRECEDENCE = ("grammar", "limit", "name")


def faults_in_tiles(T: int, placed: dict) -> bytes:
    """A text of three tiles and a bit; tile t holds the line placed[t] (a fault of FAULTS), or none, 100 bytes in."""
    out, size, first = [], 0, 1
    for t in range(3):
        pad, n = s_block(t * T + 100 - size, first)
        first += n
        out += [pad, placed.get(t, b""), b"P\tok%d\t1+,2-\t*\n" % t]
        size = sum(map(len, out))
    text = b"".join(out) + TAIL
    for t, line in placed.items():
        assert text[t * T + 100:].startswith(line) and (t * T + 100 + len(line)) // T == t
    return text


def precedence_pairs() -> dict:
    """id -> (class a, line a, class b, line b): every two faults of different classes."""
    out = {}
    for i, ca in enumerate(PRECEDENCE):
        for cb in PRECEDENCE[i + 1:]:
            for na, la in FAULTS[ca].items():
                for nb, lb in FAULTS[cb].items():
                    out["%s (%s) and %s (%s)" % (ca, na, cb, nb)] = (ca, la, cb, lb)
    return out


def precedence_triples() -> dict:
    out = {}
    for ng, lg in FAULTS["grammar"].items():
        for nl, ll in FAULTS["limit"].items():
            for nn, ln in FAULTS["name"].items():
                out["%s, %s, %s" % (ng, nl, nn)] = (lg, ll, ln)
    return out


TILE_PAIRS = ((0, 1), (1, 2), (0, 2))


def pair_texts(T: int, k: int, la: bytes, lb: bytes) -> list:
    """The two faults in two of the three tiles (which two turns with k), both ways round."""
    t0, t1 = TILE_PAIRS[k % 3]
    return [faults_in_tiles(T, {t0: la, t1: lb}), faults_in_tiles(T, {t0: lb, t1: la})]


def triple_texts(T: int, lg: bytes, ll: bytes, ln: bytes) -> list:
    """One fault of each class, one a tile, in all six orders."""
    import itertools
    return [faults_in_tiles(T, dict(enumerate(p))) for p in itertools.permutations((lg, ll, ln))]


# ---- small texts ----

def small_texts(longest: int = 5) -> list:
    """Every text of at most `longest` bytes over 'S', tab, '1' and newline: 1365 of them."""
    import itertools
    return [bytes(t) for n in range(longest + 1) for t in itertools.product(b"S\t1\n", repeat=n)]


def handmade_prefixes() -> list:
    return [text[:n] for text in HANDMADE.values() for n in range(len(text))]


# ---- the item limit ----

# quantity -> a text in which it is larger than every other quantity the limit is held against (quantities(): the lines, the
# six pool totals, the header's bytes).  An overlaps field has an op for every CIGAR, so the overlaps pool is never larger
# than the alignment pool: there the two are equal and larger than the rest.  Segments, paths and links are never more than
# the lines, so those three checks cannot be told from the one on the lines.
LIMIT_TEXTS = {
    "lines": b"S\t1\tA\n" + b"L\t1\t+\t1\t-\t\n" * 9,
    "seq_data": b"S\t1\tACGTACGTACGTACGTACGT\nS\t2\tC\n",
    "optional_data": b"S\t1\tA\tLN:i:1\tzz:Z:some words\nS\t2\tC\n",
    "alignment": b"S\t1\tA\nL\t1\t+\t1\t-\t1M2N3D4I5M6N7D8I\n",
    "name_data": b"S\t1\tA\nP\ta_path_of_a_long_name\t1+\t*\n",
    "overlaps": b"S\t1\tA\nP\tp\t1+,1-\t1M,2M,3M,4M,5M,6M,7M,8M\n",
    "steps": b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+,2+,1-,2-,1+\t*\n",
    "header": b"H\tVN:Z:1.0\tzz:Z:a header of some length\nS\t1\tA\n",
}


def quantities(pools: dict) -> dict:
    """What the device route holds against the item limit, from the host parser's pools (name -> bytes, as pools_of gives them)."""
    size = {"segs": 24, "paths": 24, "links": 16, "steps": 4, "overlaps": 8, "alignment": 4}
    out = {name: len(pools[name]) // size.get(name, 1) for name in fo.POOL_ORDER}
    out["lines"] = out.pop("line_order")
    return out
