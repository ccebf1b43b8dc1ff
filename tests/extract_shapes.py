"""Planted graphs for extract, each aimed at one rule of flatgfa/src/ops/extract.rs (tests/extract_model.py restates them).

A shape gives the GFA text, the arguments of `fgfa extract`, the rule it is aimed at, the answer derived by hand (the new
segments' names in id order, the new paths' names in order) and a proof that it exercises the rule: a variant of the model
(extract_model.VARIANTS) or other arguments under which the answer must change."""
from dataclasses import dataclass, field
from typing import Optional

from oracle import flatgfa_oracle as fo


@dataclass
class Shape:
    name: str
    rule: str
    gfa: bytes
    n: int                      # -n: the segment's name
    c: int                      # -c
    d: int = 300000             # -d
    e: int = 6                  # -e
    segs: list = field(default_factory=list)    # expected segment names, in new-id order
    paths: list = field(default_factory=list)   # expected path names, in order
    variant: Optional[str] = None               # the model variant that must change the answer
    other: Optional[dict] = None                # ... or other arguments (of n, c, d, e) that must
    zero: tuple = ()                            # segment ids whose sequence is made empty (a `*` segment of length 0)

    def pools(self) -> fo.Pools:
        p = fo.parse_gfa(self.gfa)
        for s in self.zero:
            p.segs[s]["seq_end"] = p.segs[s]["seq_start"]
        return p


def _gfa(segs, paths=(), links=()):
    """segs: (name, length); paths: (name, "1+,2-"); links: "1+2+" style tuples (from, orient, to, orient)."""
    out = [b"H\tVN:Z:1.0"]
    for k, (nm, ln) in enumerate(segs):
        out.append(b"S\t%d\t%s" % (nm, (b"ACGT" * (ln // 4 + 2))[k % 4:][:ln]))
    for nm, st in paths:
        out.append(b"P\t%s\t%s\t*" % (nm, st))
    for f, fo_, t, to_ in links:
        out.append(b"L\t%d\t%s\t%d\t%s\t0M" % (f, fo_, t, to_))
    return b"\n".join(out) + b"\n"


L = lambda f, t: (f, b"+", t, b"+")  # noqa: E731
AX = [(1, 2), (2, 3)]            # A = 1 (2 bases), X = 2 (3 bases)
AXY = [(1, 2), (2, 3), (3, 4)]   # ... Y = 3 (4 bases)

SHAPES = [
    # ---- the neighbourhood (extract.rs:159-178) ----
    Shape("two_parents_lifo", "a level pops its frontier from the back: 3 is walked before 2, so 5 (link 3) and 4 (link 4) are met in that order",
          _gfa([(k, 2) for k in range(1, 6)], [(b"p", b"1+,2+,4+,5+,3+")], [L(1, 2), L(1, 3), L(2, 4), L(3, 5), L(3, 4)]),
          n=1, c=2, e=0, segs=[1, 2, 3, 5, 4], paths=[b"p:0-10"], variant="fifo"),
    Shape("to_from_link", "incident_seg follows a link from its `to` end back to its `from` end",
          _gfa(AX, [(b"p", b"2+,1+")], [L(2, 1)]), n=1, c=1, segs=[1, 2], paths=[b"p:0-5"], variant="from_only"),
    Shape("self_loops", "a self-loop yields the popped segment itself (a no-op) and is kept as a link",
          _gfa(AXY, [(b"p", b"1+,1+,2-")], [L(1, 1), L(1, 2), L(2, 2), L(3, 3)]), n=1, c=5, segs=[1, 2], paths=[b"p:0-7"],
          other={"c": 0}),
    Shape("c_zero", "-c 0: the origin alone, with its own links and its runs of steps",
          _gfa(AX, [(b"p", b"1+,2+,1-")], [L(1, 2), L(1, 1)]), n=1, c=0, e=0, segs=[1], paths=[b"p:0-2", b"p:5-7"], other={"c": 1}),
    Shape("c_past_diameter", "-c far past the diameter: the levels run dry and the whole component is taken",
          _gfa([(k, 1) for k in range(1, 6)], [(b"p", b"1+,2+,3+,4+,5+")], [L(1, 2), L(2, 3), L(3, 4)]),
          n=1, c=10 ** 12, e=0, segs=[1, 2, 3, 4], paths=[b"p:0-4"], other={"c": 2}),
    Shape("duplicate_names", "find_seg takes the first segment of that name: id 0 (2 bases), not id 2 (4 bases)",
          _gfa([(5, 2), (7, 3), (5, 4), (9, 1)]), n=5, c=0, segs=[5], paths=[], variant="last_name"),
    # ---- merging (extract.rs:65-98, 181-185); the set is {A} unless said otherwise ----
    Shape("leading_gap", "the gap before the first member step is never filled (ignore_path)",
          _gfa(AX, [(b"p", b"2+,1+,2+,1+")]), n=1, c=0, d=4, segs=[1], paths=[b"p:3-5", b"p:8-10"], variant="fill_leading"),
    Shape("reentry_at_D", "re-entry at a step that starts exactly at D fills the gap (<=)",
          _gfa(AX, [(b"p", b"1+,2+,1+")]), n=1, c=0, d=5, segs=[1, 2], paths=[b"p:0-7"], variant="lt"),
    Shape("reentry_at_D_plus_1", "re-entry one base past D does not, although the gap itself is only 3 long: the bound is on the position",
          _gfa(AX, [(b"p", b"1+,2+,1+")]), n=1, c=0, d=4, segs=[1], paths=[b"p:0-2", b"p:5-7"], variant="gap_length"),
    Shape("open_gap_unclosed", "A X X: the gap is still open at the path's end and fills nothing",
          _gfa(AX, [(b"p", b"1+,2+,2+")]), n=1, c=0, segs=[1], paths=[b"p:0-2"], variant="fill_trailing"),
    Shape("open_gap_closed", "A X X A: the same gap, closed by the re-entry, fills X once",
          _gfa(AX, [(b"p", b"1+,2+,2+,1+")]), n=1, c=0, segs=[1, 2], paths=[b"p:0-10"], other={"e": 0}),
    Shape("fill_same_path", "A X A Y X: the fill of X makes the last step a member, which closes the gap of Y",
          _gfa(AXY, [(b"p", b"1+,2+,1+,3+,2+")]), n=1, c=0, e=1, segs=[1, 2, 3], paths=[b"p:0-14"], variant="frozen_path"),
    Shape("fill_later_path", "p fills X; q = A Y X then re-enters at X in the same sweep",
          _gfa(AXY, [(b"p", b"1+,2+,1+"), (b"q", b"1+,3+,2+")]), n=1, c=0, e=1, segs=[1, 2, 3], paths=[b"p:0-7", b"q:0-9"],
          variant="frozen_sweep"),
    Shape("fill_earlier_path", "q fills X after p = A Y X was walked: p re-enters at X only in sweep 2",
          _gfa(AXY, [(b"p", b"1+,3+,2+"), (b"q", b"1+,2+,1+")]), n=1, c=0, segs=[1, 2, 3], paths=[b"p:0-9", b"q:0-7"],
          variant="one_sweep"),
    Shape("e_zero", "-e 0: no sweep at all",
          _gfa(AX, [(b"p", b"1+,2+,1+")]), n=1, c=0, e=0, segs=[1], paths=[b"p:0-2", b"p:5-7"], other={"e": 1}),
    Shape("zero_length_in_gap", "A X Z A with Z empty: A re-enters at 5 = D, and the empty segment is filled with X",
          _gfa(AXY, [(b"p", b"1+,2+,3+,1+")]), n=1, c=0, d=5, zero=(2,), segs=[1, 2, 3], paths=[b"p:0-7"], variant="lt"),
    Shape("zero_length_reentry", "the set is {A, Z}, Z empty: A X Z re-enters at Z, which starts at 5 = D, and ends at 5",
          _gfa(AXY, [(b"p", b"1+,2+,3+")], [L(1, 3)]), n=1, c=1, d=5, zero=(2,), segs=[1, 3, 2], paths=[b"p:0-5"], variant="lt"),
    # ---- subpaths (extract.rs:102-134) ----
    Shape("path_never_enters", "a path that never touches the neighbourhood gives no subpath",
          _gfa(AXY, [(b"p", b"2+,3+"), (b"q", b"3-,1+")]), n=1, c=0, segs=[1], paths=[b"q:4-6"], other={"n": 2}),
    Shape("path_ends_inside", "a run still open at the path's end ends at the path's length",
          _gfa(AXY, [(b"p", b"3+,2+,1-")]), n=1, c=0, segs=[1], paths=[b"p:7-9"], other={"n": 3}),
    Shape("several_runs", "each maximal run of member steps is a path of its own, named by its base positions",
          _gfa(AXY, [(b"p", b"1+,2+,1-,1+,3+,1+")], [L(1, 2), L(2, 3)]), n=1, c=0, e=0, segs=[1],
          paths=[b"p:0-2", b"p:5-9", b"p:13-15"], other={"c": 1}),
]
BY_NAME = {s.name: s for s in SHAPES}
assert len(BY_NAME) == len(SHAPES)
