"""The GFA printer (flatgfa/src/print.rs) restated over the eleven pools, for the tests of the device printer: every rule
carries the lines of print.rs it restates.  `pools` is anything with the pools as attributes in FlatGFA.pool's layout
(oracle.flatgfa_oracle.Pools, or pools_of(g) below).  Where the reference panics the model raises PrintError with the
sentence flatgfa_print_gfa gives."""
from types import SimpleNamespace

from pollen_amd.flatgfa import POOLS

H, S, P, L = 0, 1, 2, 3  # LineKind, flatgfa.rs:262-269
LETTERS = b"MNDI"  # print.rs:16-19: Match, Gap, Insertion, Deletion


class PrintError(Exception):
    pass


def pools_of(g):
    return SimpleNamespace(**{n: g.pool(n) for n in POOLS})


def alignment(p, start, end) -> bytes:
    if start == end:  # print.rs:26-28
        return b"0M"
    # print.rs:29-31: {len}{op} per op; the length is the word above its low byte, the opcode the byte (flatgfa.rs:213-249)
    return b"".join(b"%d%c" % (int(op) >> 8, LETTERS[int(op) & 3]) for op in p.alignment[start:end])


def handle(p, bits) -> bytes:
    bits = int(bits)
    return b"%d%c" % (int(p.segs["name"][bits >> 1]), b"-"[0] if bits & 1 else b"+"[0])  # print.rs:41-43, :7-8


def segment(p, i) -> bytes:
    s = p.segs[i]
    out = b"S\t%d\t" % int(s["name"]) + p.seq_data[s["seq_start"]:s["seq_end"]].tobytes()  # print.rs:90
    if s["opt_start"] != s["opt_end"]:  # print.rs:91-93
        out += b"\t" + p.optional_data[s["opt_start"]:s["opt_end"]].tobytes()
    return out


def path(p, i) -> bytes:
    r = p.paths[i]
    out = b"P\t" + p.name_data[r["name_start"]:r["name_end"]].tobytes() + b"\t"  # print.rs:49
    steps = p.steps[r["steps_start"]:r["steps_end"]]
    if len(steps) == 0:  # print.rs:51: steps[0]
        raise PrintError("print: path with no steps")
    out += b",".join(handle(p, h) for h in steps)  # print.rs:51-54
    out += b"\t"  # print.rs:55
    if r["ov_start"] == r["ov_end"]:  # print.rs:57-58
        return out + b"*"
    # print.rs:60-63
    return out + b",".join(alignment(p, o["start"], o["end"]) for o in p.overlaps[r["ov_start"]:r["ov_end"]])


def link(p, i) -> bytes:
    r = p.links[i]
    f, t = int(r["from_"]), int(r["to"])
    return b"L\t%d\t%c\t%d\t%c\t" % (int(p.segs["name"][f >> 1]), b"-+"[1 - (f & 1)], int(p.segs["name"][t >> 1]),
                                     b"-+"[1 - (t & 1)]) + alignment(p, r["ov_start"], r["ov_end"])  # print.rs:71-83


def header(p) -> bytes:
    return b"H\t" + p.header.tobytes()  # print.rs:108, :130


def lines(p):
    """The lines in print order, without their newlines."""
    if len(p.line_order) == 0:  # print.rs:147-148, write_normalized :128-142
        if len(p.header):  # print.rs:129-131
            yield header(p)
        for i in range(len(p.segs)):
            yield segment(p, i)
        for i in range(len(p.paths)):
            yield path(p, i)
        for i in range(len(p.links)):
            yield link(p, i)
        return
    si = pi = li = 0  # write_preserved, print.rs:99-125
    for kind in p.line_order.tolist():
        if kind == H:
            if len(p.header) == 0:  # print.rs:107
                raise PrintError("print: empty header")
            yield header(p)
        elif kind == S:
            if si >= len(p.segs):  # print.rs:111
                raise PrintError("print: too few segments")
            yield segment(p, si)
            si += 1
        elif kind == P:
            if pi >= len(p.paths):  # print.rs:115
                raise PrintError("print: too few paths")
            yield path(p, pi)
            pi += 1
        elif kind == L:
            if li >= len(p.links):  # print.rs:119
                raise PrintError("print: too few links")
            yield link(p, li)
            li += 1
        else:  # (no LineKind: flatgfa.rs:262-269)
            raise PrintError("print: bad line kind")


def gfa(p) -> bytes:
    return b"".join(ln + b"\n" for ln in lines(p))  # writeln!, print.rs:108-139
