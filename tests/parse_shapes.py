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
