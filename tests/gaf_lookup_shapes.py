"""Generators of GAF texts (and graphs) that put the GAF lookup's kernels on their edges, with the answers they must give.

Used by tests/test_gpu_gaf_lookup*.py on the GPU; tests/test_gaf_lookup_shapes.py pins every generator -- and every closed
form that stands in for the model at large size -- to tests/gaf_lookup_model.py on the CPU.

The device's units: a wave walks a line 64 bytes a step; the line index counts '\\n' in tiles of 16 KiB (64 consecutive bytes
per lane); the `-s` text is gathered in tiles of 16 KiB of output, 16 bytes per lane and row.
"""
from __future__ import annotations

import random
from typing import List, Sequence, Tuple

import gaf_lookup_model as M

STEP, TILE, OUT_TILE = 64, 16384, 16384


def gaf_line(name: bytes, path: bytes, start, end, tail: bytes = b"60\tcg:Z:1M", f1: bytes = b"10") -> bytes:
    """A GAF record: the 12 mandatory fields, the ones the lookup ignores filled with small numbers."""
    return b"\t".join([name, f1, b"0", b"10", b"+", path, b"100", str(start).encode() if not isinstance(start, bytes) else start,
                       str(end).encode() if not isinstance(end, bytes) else end, b"10", b"10", tail]) + b"\n"


def path_of(g: M.Graph, walk: Sequence[Tuple[int, bool]]) -> bytes:
    return b"".join((b">" if fwd else b"<") + str(g.names[sid]).encode() for sid, fwd in walk)


def random_reads(g: M.Graph, seed: int, n_reads: int, max_tokens: int = 12) -> bytes:
    """Seeded random walks over the segments of `g`, forward and backward handles, `start` <= `end` inside the walk (now and then
    exactly on a segment's end, at 0, or at the walk's end)."""
    rnd = random.Random(seed)
    S = len(g.names)
    out = []
    for r in range(n_reads):
        walk = [(rnd.randrange(S), rnd.random() < 0.5) for _ in range(rnd.randint(1, max_tokens))]
        total = sum(len(g.seqs[s]) for s, _ in walk)
        edges = [0]
        for s, _ in walk:
            edges.append(edges[-1] + len(g.seqs[s]))
        pick = lambda: rnd.choice(edges) if rnd.random() < 0.3 else rnd.randint(0, total)  # noqa: E731
        a, b = sorted((pick(), pick()))
        out.append(gaf_line(b"read%d" % r, path_of(g, walk), a, b))
    return b"".join(out)


def padded_reads(g: M.Graph, seed: int, boundary: int, span: int = 40) -> bytes:
    """Reads laid out so that, over the `span` variants concatenated, every part of a record -- the '\\n', each tab, the digits of
    `start` and `end`, a token's '>' and its digits -- falls on both sides of a multiple of `boundary` bytes: each variant starts
    with a filler read whose name is padded to end k bytes short of the boundary."""
    rnd = random.Random(seed)
    S = len(g.names)
    out, at = [], 0
    for k in range(span):
        filler_base = gaf_line(b"", b">%d" % g.names[0], 0, 0)
        want = (-(at + len(filler_base) + k)) % boundary
        filler = gaf_line(b"p" * want, b">%d" % g.names[0], 0, 0)
        walk = [(rnd.randrange(S), rnd.random() < 0.5) for _ in range(rnd.randint(2, 6))]
        total = sum(len(g.seqs[s]) for s, _ in walk)
        a, b = sorted((rnd.randint(0, total), rnd.randint(0, total)))
        rec = gaf_line(b"edge%d" % k, path_of(g, walk), a, b)
        out += [filler, rec]
        at += len(filler) + len(rec)
    return b"".join(out)


def long_path_line(g: M.Graph, n_tokens: int, start: int, end: int, name: bytes = b"long") -> bytes:
    """One read whose path cycles through all segments, forward on even tokens and backward on odd ones."""
    S = len(g.names)
    return gaf_line(name, path_of(g, [(t % S, t % 2 == 0) for t in range(n_tokens)]), start, end)


def long_path_count(n_tokens: int) -> int:
    """The events of long_path_line: one per token."""
    return n_tokens


def many_short_lines(name_of_seg0: int, n: int) -> bytes:
    """n identical short reads over segment 0: Partial(0, 1) each when the segment has at least two bases."""
    return gaf_line(b"r", b">%d" % name_of_seg0, 0, 1, tail=b"0", f1=b"1") * n


def many_short_lines_seqs(seg0: bytes, n: int) -> bytes:
    """The `-s` text of many_short_lines (closed form; needs len(seg0) >= 2)."""
    return (b"r\t" + seg0[0:1] + b"\n") * n


def big_segment_gfa(n_bases: int, seed: int = 7) -> Tuple[bytes, bytes]:
    """A graph of three segments -- 1: 5 bases, 2: `n_bases` seeded bases with lower case and N among them, 3: 0 bases (`*` is not
    used: an empty sequence field) -- as GFA text, and segment 2's bases."""
    rnd = random.Random(seed)
    big = bytes(rnd.choice(b"ACGTACGTACGTacgtN") for _ in range(n_bases))
    return b"H\tVN:Z:1.0\nS\t1\tGATTA\nS\t2\t" + big + b"\nS\t3\t\n", big


def big_segment_reads(n_bases: int) -> bytes:
    """Reads through the big segment in both orientations: starting inside segment 1, covering all of 2 (and the empty 3), ending
    inside the last; and one that starts and ends inside 2."""
    a, b = n_bases // 3 + 1, n_bases - n_bases // 5
    return (gaf_line(b"fwd", b">1>2>3>1", 2, 5 + n_bases + 3) + gaf_line(b"bwd", b"<1<3<2<1", 1, 5 + n_bases + 2) +
            gaf_line(b"in_f", b">2", a, b) + gaf_line(b"in_b", b"<2", a, b))


def big_segment_seqs(big: bytes) -> bytes:
    """The `-s` text of big_segment_reads (closed form, pinned to the model at small size)."""
    n = len(big)
    a, b = n // 3 + 1, n - n // 5
    s1 = b"GATTA"
    r1 = M.revcomp(s1)
    rb = M.revcomp(big)
    return (b"fwd\t" + s1[2:] + big + s1[:3] + b"\n" + b"bwd\t" + r1[1:] + rb + r1[:2] + b"\n" +
            b"in_f\t" + big[a:b] + b"\n" + b"in_b\t" + rb[a:b] + b"\n")


def zero_byte_events(g_names: Sequence[int], n_none: int) -> bytes:
    """A read whose first token covers everything asked for, followed by `n_none` tokens that give nothing: events of zero bytes
    between (and across) output tiles when the line is repeated."""
    path = b">%d" % g_names[0] + b"".join(b"<%d" % g_names[t % len(g_names)] for t in range(n_none))
    return gaf_line(b"z", path, 0, 1)


BAD_LINES = {
    # name -> (line without its '\n', the code it must give)
    "empty": (b"", "parse"),
    "eight_tabs": (b"a\t1\t0\t1\t+\t>1\t8\t0\t1", "parse"),
    "no_start": (b"a\t1\t0\t1\t+\t>1\t8\t\t1\t1\t1\t0", "parse"),
    "start_not_digits": (b"a\t1\t0\t1\t+\t>1\t8\tx\t1\t1\t1\t0", "parse"),
    "start_digits_then_junk": (b"a\t1\t0\t1\t+\t>1\t8\t0x\t1\t1\t1\t0", "parse"),
    "no_end": (b"a\t1\t0\t1\t+\t>1\t8\t0\t\t1\t1\t0", "parse"),
    "end_is_last": (b"a\t1\t0\t1\t+\t>1\t8\t0\t1", "parse"),
    "unknown_name": (b"a\t1\t0\t1\t+\t>1>999999\t8\t0\t1\t1\t1\t0", "bounds"),
    "name_zero": (b"a\t1\t0\t1\t+\t>0\t8\t0\t1\t1\t1\t0", "bounds"),
}


def lines_with_tabs(n_tabs: int, seed: int) -> List[bytes]:
    """Generated lines of `n_tabs` tabs whose fields are drawn from digits, letters, the empty string and a path."""
    rnd = random.Random(seed * 131 + n_tabs)
    pool = [b"", b"0", b"7", b"12", b"x", b"1x", b"x1", b">1", b"+", b" 3", b"007"]
    return [b"\t".join(rnd.choice(pool) for _ in range(n_tabs + 1)) for _ in range(40)]
