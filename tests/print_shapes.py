"""Graphs for the tests of the device GFA printer: handmade texts that use every rule of print.rs, and builders for the
seams of the device layout (16 KiB tiles, 4 MiB pieces, item chunks).  Texts are parsed by the library; pools that no text
gives (a line_order shorter than its pools, paths that share steps, a path without steps) are written as a .flatgfa
container by oracle.flatgfa_oracle.dump_flatgfa.

The second half holds the shapes of tests/test_gpu_print_seams.py.  Each builder takes the size it has to hit and asserts
the property it exists for (a length that is a multiple of a tile, the bytes a field leaves in the next tile, the item a
chunk begins with) from the text alone: item_sizes, pieces, long_fields and clipped restate how the device cuts a text into
items, chunks, pieces and tiles.  tests/test_print_model.py pins every one of them on the host."""
import dataclasses

import numpy as np

from oracle import flatgfa_oracle as fo

TILE = 16384
PIECE = 4 << 20
U64_MAX = (1 << 64) - 1

HANDMADE = {
    "plain": b"H\tVN:Z:1.0\nS\t1\tACGT\nS\t2\tAC\nS\t3\tG\nP\tp\t1+,2+,3-\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t-\t0M\n",
    "header in the middle": b"S\t1\tACGT\nS\t2\tAC\nH\tVN:Z:1.0\nL\t1\t+\t2\t-\t2M\nP\tx\t1+,2-\t*\n",
    "P before S": b"P\tfirst\t2-,1+,2+\t*\nL\t2\t-\t1\t+\t0M\nS\t1\tA\nS\t2\tCC\nP\tsecond\t1-\t*\n",
    "CIGARs of several ops": b"S\t1\tACGTACGTAC\nS\t2\tGTACGTACGT\nL\t1\t+\t2\t+\t4M2D1I3N\nL\t2\t-\t1\t-\t255M\nL\t1\t-\t2\t+\t0M1N\n"
                             b"P\tp\t1+,2+\t*\n",
    "path overlaps": b"S\t1\tAAAA\nS\t2\tCCCC\nS\t3\tGGGG\nP\tq\t1+,2-,3+\t2M,10M3D\nP\tr\t3-,2+\t4M\nP\ts\t1+\t*\n",
    "optional fields": b"H\tVN:Z:1.0\nS\t1\tACGT\tLN:i:4\tRC:i:12\nS\t2\t*\nS\t3\tG\txx:Z:some words here\nP\tp\t1+,3+\t*\n",
    "a 20-digit name": b"S\t18446744073709551615\tAC\nS\t10000000000000000000\tG\nS\t9999999999999999999\tT\n"
                       b"L\t18446744073709551615\t+\t10000000000000000000\t-\t1M\n"
                       b"P\tbig\t18446744073709551615+,9999999999999999999-,10000000000000000000+\t*\n",
    "only a header": b"H\tVN:Z:1.0\n",
    "no newline at the end": b"S\t7\tACGT\nP\tp\t7+\t*",
}


def bases(n: int, seed: int = 1) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def one_long_segment(n: int) -> bytes:
    """A short segment, one of n bases, a short one: the long line's ends fall wherever n puts them."""
    return b"S\t1\tAC\nS\t2\t" + bases(n) + b"\nS\t3\tG\nP\tp\t1+,2-,3+\t*\nL\t1\t+\t2\t+\t0M\n"


def long_optional(n: int) -> bytes:
    return b"S\t1\tACGT\tzz:Z:" + bases(n, 2).lower() + b"\nS\t2\tA\nL\t1\t+\t2\t+\t0M\nP\tp\t1+,2+\t*\n"


def path_name(n: int) -> bytes:
    name = (b"path_name." * (n // 10 + 1))[:n]
    return b"S\t1\tACGT\nS\t2\tC\nP\t" + name + b"\t1+,2-\t*\nP\tafter\t2+\t*\n"


def digit_names() -> bytes:
    """Segment names on both sides of every power of ten, and 2^64 - 1; a path and links through them all."""
    names = [9]
    for d in range(1, 20):
        names += [10 ** d - 1, 10 ** d]
    names = sorted(set(names)) + [U64_MAX]
    out = [b"S\t%d\tA" % n for n in names]
    out += [b"L\t%d\t+\t%d\t-\t%dM" % (a, b, i) for i, (a, b) in enumerate(zip(names, names[1:]))]
    out.append(b"P\tp\t" + b",".join(b"%d%s" % (n, b"+-"[i % 2:i % 2 + 1]) for i, n in enumerate(names)) + b"\t*")
    return b"\n".join(out) + b"\n"


def long_overlaps(n_ops: int) -> bytes:
    """A path whose overlaps field is longer than a tile (n_ops alignments of two ops each), between two short paths."""
    steps = b",".join(b"%d%s" % (1 + i % 2, b"+-"[i % 2:i % 2 + 1]) for i in range(n_ops + 1))
    ovl = b",".join(b"%dM%dD" % (1 + i % 255, i % 13) for i in range(n_ops))
    return b"S\t1\tAC\nS\t2\tGT\nP\ta\t1+\t*\nP\tlong\t" + steps + b"\t" + ovl + b"\nP\tz\t2-,1+\t3M\n"


def long_cigar(n_ops: int, lead: int) -> bytes:
    """A link CIGAR of n_ops ops that starts `lead` bases into the text's first tile, so that it lies across a tile edge."""
    cigar = b"".join(b"%d%c" % (i % 256, b"MNDI"[i % 4]) for i in range(n_ops))
    return b"S\t1\t" + bases(lead) + b"\nS\t2\tC\nL\t1\t+\t2\t-\t" + cigar + b"\nL\t2\t+\t1\t+\t0M\nP\tp\t1+,2-\t*\n"


def alternating(n: int) -> bytes:
    """A preserved order that changes kind with every line: S, L, P, S, L, P, ... with a header in between."""
    out = [b"S\t1\tA"]
    for i in range(2, n + 2):
        out += [b"S\t%d\t%s" % (i, bases(1 + i % 5, i)), b"L\t%d\t+\t%d\t-\t%dM" % (i - 1, i, i % 3), b"P\tp%d\t%d+,%d-\t*" % (i, i - 1, i)]
        if i == n // 2:
            out.append(b"H\tVN:Z:1.0")
    return b"\n".join(out) + b"\n"


# ---- pools that no text gives ----

def with_pools(p: fo.Pools, **changed) -> fo.Pools:
    return dataclasses.replace(p, **changed)


def short_line_order(text: bytes, keep: int) -> fo.Pools:
    """The first `keep` lines of the order only: the pools hold more than is printed."""
    p = fo.parse_gfa(text)
    return with_pools(p, line_order=p.line_order[:keep].copy())


def normalized(text: bytes) -> fo.Pools:
    p = fo.parse_gfa(text)
    return with_pools(p, line_order=p.line_order[:0].copy())


def shared_steps(text: bytes) -> fo.Pools:
    """Every path takes the first path's steps span."""
    p = fo.parse_gfa(text)
    paths = p.paths.copy()
    paths["steps_start"], paths["steps_end"] = paths["steps_start"][0], paths["steps_end"][0]
    return with_pools(p, paths=paths)


def path_without_steps(text: bytes, which: int) -> fo.Pools:
    p = fo.parse_gfa(text)
    paths = p.paths.copy()
    paths["steps_end"][which] = paths["steps_start"][which]
    return with_pools(p, paths=paths)


def bad_step(text: bytes) -> fo.Pools:
    p = fo.parse_gfa(text)
    steps = p.steps.copy()
    steps[-1] = (len(p.segs) + 3) << 1
    return with_pools(p, steps=steps)


def wide_ops(text: bytes) -> fo.Pools:
    """Op lengths up to the 24 bits a word holds (the parser stops at 255, flatgfa.rs:228)."""
    p = fo.parse_gfa(text)
    a = p.alignment.copy()
    for i in range(len(a)):
        a[i] = (int(a[i]) & 0xFF) | ((((1 << 24) - 1) >> (3 * (i % 8))) << 8)
    return with_pools(p, alignment=a)


def order_of(text: bytes, order) -> fo.Pools:
    p = fo.parse_gfa(text)
    return with_pools(p, line_order=np.array(order, np.uint8))


# ---- items, chunks and pieces: what the device cuts a text into ----

def item_sizes(text: bytes) -> list:
    """The bytes of every item of a printed text, in order: an H, S or L line is one item, a P line one per step -- the first
    with "P\\t{name}\\t", the last with the overlaps field and the newline, each with its ',' or tab."""
    assert text.endswith(b"\n")
    out = []
    for ln in text[:-1].split(b"\n"):
        if ln[:1] != b"P":
            out.append(len(ln) + 1)
            continue
        _, name, steps, ovl = ln.split(b"\t")
        sizes = [len(s) + 1 for s in steps.split(b",")]
        sizes[0] += 3 + len(name)
        sizes[-1] += len(ovl) + 1
        out += sizes
    assert sum(out) == len(text)
    return out


def chunk_bytes(sizes: list, chunk: int) -> list:
    """The bytes of every chunk of `chunk` items."""
    return [sum(sizes[i:i + chunk]) for i in range(0, len(sizes), chunk)]


def pieces(sizes: list, chunk: int = 1 << 20) -> list:
    """The piece lengths a sink sees: every chunk leaves in pieces of PIECE bytes and a rest, and a piece is never empty."""
    out = []
    for n in chunk_bytes(sizes, chunk):
        out += [PIECE] * (n // PIECE) + ([n % PIECE] if n % PIECE else [])
    return out


def line_items(text: bytes) -> list:
    """(first item, items) of every line of a printed text."""
    out, at = [], 0
    for ln in text[:-1].split(b"\n"):
        n = len(ln.split(b"\t")[2].split(b",")) if ln[:1] == b"P" else 1
        out.append((at, n))
        at += n
    return out


def long_fields(text: bytes) -> list:
    """(kind, start, end) of every field the device copies from a pool: a segment's bases and its optional fields, a path's
    name, the header."""
    out, at = [], 0
    for ln in text[:-1].split(b"\n"):
        f = ln.split(b"\t")
        if f[0] == b"H":
            out.append(("header", at + 2, at + len(ln)))
        elif f[0] == b"S":
            seq = at + 3 + len(f[1])
            out.append(("segment", seq, seq + len(f[2])))
            if len(f) > 3:
                out.append(("optional", seq + len(f[2]) + 1, at + len(ln)))
        elif f[0] == b"P":
            out.append(("path name", at + 2, at + 2 + len(f[1])))
        at += len(ln) + 1
    return out


def clipped(span, tile: int) -> int:
    """How many bytes of (start, end) lie in tile `tile`."""
    return max(0, min(span[-1], (tile + 1) * TILE) - max(span[-2], tile * TILE))


def long_copies(text: bytes, tile: int) -> int:
    """How many copies of tile `tile` go the workgroup's way: more than 64 bytes after clipping to the tile."""
    return sum(clipped(f, tile) > 64 for f in long_fields(text))


# ---- seam 1: a text, a chunk or a piece that ends on a multiple ----

_BASES = bases(1 << 16, 7)
TAIL = b"L\t1\t+\t2\t-\t3M\nP\tend\t1+,2-,1+\t2M,1N\n"


def s_block(size: int, first: int = 1, width: int = 97):
    """S lines named first, first + 1, ... of 1..width bases that make exactly `size` bytes, the last one padded to get
    there.  Returns the text and how many lines it has."""
    out, name, left = [], first, size
    while True:
        n = 1 + (name * 37) % width
        head = b"S\t%d\t" % name
        if left - (len(head) + n + 1) < len(head) + 3:  # no room for a line behind this one: it takes the rest
            n = left - len(head) - 1
            assert 1 <= n <= len(_BASES)
        at = (name * 131) % (len(_BASES) - n + 1)
        out.append(head + _BASES[at:at + n] + b"\n")
        left -= len(out[-1])
        if not left:
            text = b"".join(out)
            assert len(text) == size
            return text, name - first + 1
        name += 1


def exact_text(size: int, width: int = 97) -> bytes:
    """A text of exactly `size` bytes that ends in a link and a path with an overlaps field."""
    text = s_block(size - len(TAIL), 1, width)[0] + TAIL
    assert len(text) == size
    return text


def chunk_then_more(size: int, width: int = 97):
    """A text whose first `chunk` items are exactly `size` bytes, and which goes on behind them.  Returns (text, chunk)."""
    head, n = s_block(size, 1, width)
    more = TAIL + s_block(3000, n + 1)[0] + b"P\tafter\t%d+,1-\t*\n" % (n + 1)
    text = head + more
    assert sum(item_sizes(text)[:n]) == size and len(item_sizes(text)) > n
    return text, n


# ---- seam 3: paths to cut ----

def cut_paths(k: int) -> bytes:
    """"path overlaps" grown: paths of k steps, and one of one step, each with an overlaps field of several alignments of
    several ops."""
    ovl = b"2M,10M3N,255M1N7M,4M"
    def steps(n, seed):
        return b",".join(b"%d%s" % (1 + (i * seed) % 3, b"+-"[(i + seed) % 2:(i + seed) % 2 + 1]) for i in range(n))
    return (b"S\t1\tAAAA\nS\t2\tCCCC\nS\t3\tGGGG\nP\tq\t" + steps(k, 1) + b"\t" + ovl + b"\nL\t1\t+\t2\t-\t2M\nP\tone\t3-\t" + ovl
            + b"\nP\tr\t" + steps(k + 3, 2) + b"\t4M1N,12M\nS\t4\tT\nP\tlast\t" + steps(k, 5) + b"\t" + ovl + b"\n")


def cuts(sizes: list, chunk: int) -> set:
    """The items a chunk begins with."""
    return set(range(0, len(sizes), chunk))


# ---- seams 4 and 6: a pool copy across a tile's edge ----

def _field_line(kind: str, n: int) -> bytes:
    if kind == "segment":
        return b"S\t2\t" + bases(n, 3) + b"\n"
    if kind == "optional":
        return b"S\t2\tACGT\tzz:Z:" + bases(n - 5, 4).lower() + b"\n"
    if kind == "path name":
        return b"P\t" + (b"path_name." * (n // 10 + 1))[:n] + b"\t1+,3-\t*\n"
    assert kind == "header"
    return b"H\tVN:Z:1.0\tzz:Z:" + bases(n - 14, 5).lower() + b"\n"


def straddle(kind: str, before: int, after: int) -> bytes:
    """A text in which the `kind` field ("segment", "optional", "path name", "header") has its last `after` bytes behind
    the first tile edge and `before` bytes in front of it; a padded segment in front of its line puts it there."""
    line = _field_line(kind, before + after)
    (lead,) = [f[1] for f in long_fields(line) if f[0] == kind]  # where the field begins in its line
    pad = TILE - before - lead - 5  # "S\t1\t", the padding, its newline
    text = b"S\t1\t" + bases(pad, 6) + b"\n" + line + b"S\t3\tG\nL\t1\t+\t3\t-\t0M\nP\tp\t3+,1-\t*\n"
    (span,) = [f for f in long_fields(text) if f[0] == kind and f[1] == TILE - before]
    assert span[2] - span[1] == before + after and clipped(span, 0) == before
    assert sum(clipped(span, t) for t in range(1, 4)) == after
    return text


def leaves_in_next_tile(make, kind: str, rest: int) -> bytes:
    """make(n) -- one_long_segment, long_optional, path_name -- sized so that its long field ends `rest` bytes into the
    second tile."""
    def span(text):
        return max((f for f in long_fields(text) if f[0] == kind), key=lambda f: f[2] - f[1])
    n = TILE
    n += TILE + rest - span(make(n))[2]
    text = make(n)
    assert span(text)[1] < TILE and clipped(span(text), 1) == rest
    return text


# ---- seam 5: many long copies a tile ----

def many_long(count: int, optional: bool = False) -> fo.Pools:
    """`count` S lines of 65 bases under one-digit names (pools: a text would need the names apart), each with a 65-byte
    optional field if asked: 70 or 136 bytes a line, every one a long copy or two."""
    opt = b"\tzz:Z:" + b"x" * 60 if optional else b""
    p = fo.parse_gfa(b"".join(b"S\t%d\t%s%s\n" % (i + 1, _BASES[67 * i % 60000:67 * i % 60000 + 65], opt) for i in range(count)))
    segs = p.segs.copy()
    segs["name"] = 1 + np.arange(count) % 9
    return with_pools(p, segs=segs)


# ---- seam 7: more than 2^32 bytes of text ----

def aliased_segments(n_segs: int, pool: int) -> fo.Pools:
    """n_segs segments that all alias one sequence span of `pool` bases; a path and a link follow the last segment but one, so
    that with 65 segments over 2^26 bases they lie just past byte 2^32."""
    p = fo.parse_gfa(b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-\t*\nL\t1\t+\t2\t-\t0M\n")
    segs = np.zeros(n_segs, fo.SEG_DT)
    segs["name"], segs["seq_end"] = 1 + np.arange(n_segs), pool
    order = np.array([1] * (n_segs - 1) + [2, 3, 1], np.uint8)
    seq = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(9).integers(0, 4, pool, dtype=np.uint8)]
    return with_pools(p, segs=segs, seq_data=seq, line_order=order)


def aliased_lines(p: fo.Pools) -> list:
    """(length, head, pool span or None, tail) of every line of aliased_segments' text: the closed form of the text."""
    import print_model as pm
    out, si = [], 0
    for kind in p.line_order.tolist():
        if kind == 1:
            head, s = b"S\t%d\t" % int(p.segs["name"][si]), p.segs[si]
            out.append((len(head) + int(s["seq_end"]) - int(s["seq_start"]) + 1, head, (int(s["seq_start"]), int(s["seq_end"])), b"\n"))
            si += 1
        else:
            ln = (pm.path(p, 0) if kind == 2 else pm.link(p, 0)) + b"\n"
            out.append((len(ln), ln, None, b""))
    return out


def aliased_window(p: fo.Pools, lo: int, hi: int) -> bytes:
    """Bytes [lo, hi) of aliased_segments' text, without the text."""
    out, at = [], 0
    for n, head, span, tail in aliased_lines(p):
        if at < hi and at + n > lo:
            a, b = max(lo - at, 0), min(hi - at, n)  # within the line
            out.append(head[a:b])
            if span:
                s0 = span[0] - len(head)
                out.append(p.seq_data[max(a + s0, span[0]):max(min(b + s0, span[1]), span[0])].tobytes())
                out.append(tail[max(a - (n - 1), 0):max(b - (n - 1), 0)])
        at += n
    return b"".join(out)


# ---- seam 8: degenerate graphs ----

ONLY_SEGMENTS = b"S\t1\tACGT\nS\t2\tC\nS\t30\tGGGTTTAAA\n"
TINY = b"S\t1\tA\n"


def only_links() -> fo.Pools:
    """The L lines of a graph and the segments they name; the order keeps the L lines alone."""
    return order_of(b"S\t1\tACGT\nS\t22\tC\nS\t3\tGG\nL\t1\t+\t22\t-\t3M\nL\t22\t-\t3\t+\t0M\nL\t3\t+\t1\t+\t12M1N\n", [3, 3, 3])


def empty_sequence(text: bytes = HANDMADE["plain"], which: int = 1) -> fo.Pools:
    p = fo.parse_gfa(text)
    segs = p.segs.copy()
    segs["seq_end"][which] = segs["seq_start"][which]
    return with_pools(p, segs=segs)


def empty_path_name(text: bytes = HANDMADE["path overlaps"], which: int = 1) -> fo.Pools:
    p = fo.parse_gfa(text)
    paths = p.paths.copy()
    paths["name_end"][which] = paths["name_start"][which]
    return with_pools(p, paths=paths)


# ---- the cases test_print_model.py pins on the host and test_gpu_print_seams.py runs on the device ----

TEXT_ENDS = [TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE, PIECE, PIECE + 1, 2 * PIECE]
CHUNK_ENDS = [TILE, 2 * TILE, PIECE, PIECE + 1, 2 * PIECE]
SCAN_CHUNKS = [1023, 1024, 1025, 2049, 4096]  # around one, two and four scan tiles of 1024 items
RESTS = [63, 64, 65, 66]  # around the 64 bytes above which a clipped copy is the workgroup's
LONG_CAP = TILE // 65 + 2  # text_tiles.hpp: kLongCap


def width_for(size: int) -> int:
    """Wider lines for the texts of a piece and more: their tests are about the ends, not the line count."""
    return 97 if size < PIECE else 1500


def crossing(text: bytes, kind: str):
    """The `kind` field that lies across the first tile edge."""
    (span,) = [f for f in long_fields(text) if f[0] == kind and f[1] < TILE < f[2]]
    return span


def clipped_cases() -> dict:
    """id -> (make, kind, tile, bytes): make() gives a text, or pools, whose `kind` field across the first tile edge has
    `bytes` bytes in `tile`."""
    out = {}
    for make, kind in ((one_long_segment, "segment"), (long_optional, "optional"), (path_name, "path name")):
        for r in RESTS:
            out["%s builder leaves %d" % (kind, r)] = (lambda make=make, kind=kind, r=r: leaves_in_next_tile(make, kind, r), kind, 1, r)
    for kind in ("segment", "optional", "path name", "header"):
        for r in RESTS:
            out["%s: %d in the next tile" % (kind, r)] = (lambda kind=kind, r=r: straddle(kind, 1000, r), kind, 1, r)
            out["%s: %d in the previous tile" % (kind, r)] = (lambda kind=kind, r=r: straddle(kind, r, 1000), kind, 0, r)
    out["header across two tile edges"] = (lambda: straddle("header", 70, TILE + 500), "header", 1, TILE)
    return out


def header_first_cases() -> dict:
    """id -> make: pools in normalized order, so that a header of more than 64 bytes, or of more than a tile, comes first."""
    return {"a header of 1065 bytes first": lambda: normalized(straddle("header", 1000, 65)),
            "a header longer than a tile first": lambda: normalized(straddle("header", 100, TILE + 500))}


CUT_TEXT = cut_paths(40)


def cut_cases(text: bytes = CUT_TEXT) -> dict:
    """id -> (chunk, items that must begin a chunk): a cut just before each path's last item, just behind its first, and on
    both sides of a one-step path."""
    out = {}
    for (first, n), ln in zip(line_items(text), text[:-1].split(b"\n")):
        if ln[:1] != b"P":
            continue
        name = ln.split(b"\t")[1].decode()
        if n == 1:
            out["%s: before its one item" % name] = (first, [first])
            out["%s: behind its one item" % name] = (first + 1, [first + 1])
            out["%s: alone in a chunk" % name] = (1, [first, first + 1])
        else:
            out["%s: before its last item" % name] = (first + n - 1, [first + n - 1])
            out["%s: behind its first item" % name] = (first + 1, [first + 1])
    return out


def degenerate_cases() -> dict:
    """id -> make: a text or pools."""
    return {"only S lines": lambda: ONLY_SEGMENTS, "only S lines, normalized": lambda: normalized(ONLY_SEGMENTS),
            "only L lines": only_links, "one line of 6 bytes": lambda: TINY,
            "an empty sequence span": empty_sequence, "an empty sequence span, normalized": lambda: normalized_pools(empty_sequence()),
            "an empty path name": empty_path_name, "an empty name on a one-step path": lambda: empty_path_name(which=2)}


def normalized_pools(p: fo.Pools) -> fo.Pools:
    return with_pools(p, line_order=p.line_order[:0].copy())
