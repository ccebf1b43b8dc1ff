"""Graphs for the tests of the device GFA printer: handmade texts that use every rule of print.rs, and builders for the
seams of the device layout (16 KiB tiles, 4 MiB pieces, item chunks).  Texts are parsed by the library; pools that no text
gives (a line_order shorter than its pools, paths that share steps, a path without steps) are written as a .flatgfa
container by oracle.flatgfa_oracle.dump_flatgfa."""
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
