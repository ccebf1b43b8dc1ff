"""tests/inject_model.py: the one-pass form of inject against the line-by-line form that follows slow_odgi/inject.py, on seeded
random graphs, and both against answers worked by hand.  No GPU."""
import numpy as np
import pytest

import inject_model as im
from oracle import flatgfa_oracle as fo

A = b"S\t1\tAAAA\nS\t2\tCC\nS\t3\tGGG\nP\tp\t1+,2-,3+\t*\nP\tq\t3-,1+\t*\nL\t1\t+\t2\t-\t0M\nL\t2\t-\t3\t+\t0M\n"
# p: 1+ [0,4)  2- [4,6)  3+ [6,9)        q: 3- [0,3)  1+ [3,7)


def view(p):
    segs, paths = im.odgi_view(p)
    return [segs[str(i + 1)] for i in range(len(segs))], paths


def both(p, lines):
    a, b = im.inject(p, lines), im.inject_sequential(p, lines)
    assert im.same_pools(a, b)
    return view(a)


def random_case(rng):
    n_segs, n_paths = int(rng.integers(1, 9)), int(rng.integers(1, 5))
    text = [b"S\t%d\t%s" % (i + 1, bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 7))))) for i in range(n_segs)]
    lens = []
    for k in range(n_paths):
        hs = [(int(rng.integers(0, n_segs)), int(rng.integers(0, 2))) for _ in range(int(rng.integers(1, 11)))]
        text.append(b"P\tp%d\t%s\t*" % (k, b",".join(b"%d%s" % (s + 1, b"+-"[o:o + 1]) for s, o in hs)))
    p = fo.parse_gfa(b"\n".join(text) + b"\n")
    if rng.random() < 0.3:  # a segment of no bases
        s = int(rng.integers(0, n_segs))
        p.segs["seq_end"][s] = p.segs["seq_start"][s]
    for path in p.paths:
        hs = p.steps[int(path["steps_start"]):int(path["steps_end"])]
        lens.append(int(sum(int(p.segs["seq_end"][h >> 1]) - int(p.segs["seq_start"][h >> 1]) for h in hs)))
    lines = []
    for k in range(int(rng.integers(0, 9))):
        q = int(rng.integers(0, n_paths + 1))  # (n_paths: a path the graph lacks)
        top = lens[q] + 3 if q < n_paths else 10
        lo, hi = int(rng.integers(0, top)), int(rng.integers(0, top))
        if rng.random() < 0.7 and lo > hi:
            lo, hi = hi, lo
        lines.append((b"p%d" % q, lo, hi, b"n%d" % k))
    return p, lines


def test_forms_agree_on_random_graphs():
    rng = np.random.default_rng(20240607)
    cut_cases = new_steps = 0
    for _ in range(400):
        p, lines = random_case(rng)
        a, b = im.inject(p, lines), im.inject_sequential(p, lines)
        assert im.same_pools(a, b), (view(p), lines)
        cut_cases += len(a.segs) > len(p.segs)
        new_steps += len(a.steps) > len(p.steps)
    assert cut_cases > 100 and new_steps > 100  # (the cases are not trivial ones)


def test_cut_in_a_backward_step():
    p = fo.parse_gfa(A)
    segs, paths = both(p, [(b"p", 5, 9, b"x")])
    assert segs == ["AAAA", "C", "C", "GGG"]  # offset 1 of the step 2- is position 2 - 1 of segment 2
    assert paths == {"p": ["1+", "3-", "2-", "4+"], "q": ["4-", "1+"], "x": ["2-", "4+"]}


def test_the_same_cut_from_two_lines():
    p = fo.parse_gfa(A)
    segs, paths = both(p, [(b"p", 5, 9, b"x"), (b"p", 5, 6, b"y")])
    assert segs == ["AAAA", "C", "C", "GGG"]
    assert paths["x"] == ["2-", "4+"] and paths["y"] == ["2-"]


def test_two_cuts_in_one_segment_from_different_paths():
    p = fo.parse_gfa(A)
    segs, paths = both(p, [(b"q", 1, 3, b"z"), (b"p", 7, 9, b"w")])
    assert segs == ["AAAA", "CC", "G", "G", "G"]  # q's 3- at offset 1 is position 2, p's 3+ at offset 1 is position 1
    assert paths == {"p": ["1+", "2-", "3+", "4+", "5+"], "q": ["5-", "4-", "3-", "1+"], "z": ["4-", "3-"], "w": ["4+", "5+"]}


def test_zero_length_segment_at_low_and_at_high():
    p = fo.parse_gfa(b"S\t1\tAA\nS\t2\tC\nS\t3\tGG\nP\tp\t1+,2+,3+\t*\n")
    p.segs["seq_end"][1] = p.segs["seq_start"][1]  # p: 1+ [0,2)  2+ [2,2)  3+ [2,4)
    segs, paths = both(p, [(b"p", 2, 4, b"x"), (b"p", 0, 2, b"y"), (b"p", 2, 2, b"z")])
    assert segs == ["AA", "", "GG"]  # a segment of no bases is never cut
    assert paths["x"] == ["2+", "3+"]  # start == low: inside
    assert paths["y"] == ["1+", "2+"]  # end == high: inside
    assert paths["z"] == ["2+"]


def test_ends_on_seams_and_past_the_end():
    p = fo.parse_gfa(A)
    segs, paths = both(p, [(b"p", 4, 6, b"s"), (b"p", 6, 100, b"t"), (b"p", 9, 12, b"u"), (b"p", 7, 3, b"v"), (b"p", 3, 3, b"e")])
    assert segs == ["AAA", "A", "CC", "G", "GG"]  # only 7 and 3 are inside a step
    assert paths["s"] == ["3-"] and paths["t"] == ["4+", "5+"]
    assert paths["u"] == [] and paths["v"] == [] and paths["e"] == []
    assert paths["p"] == ["1+", "2+", "3-", "4+", "5+"]


def test_a_line_on_a_path_the_graph_lacks_is_skipped():
    p = fo.parse_gfa(A)
    assert both(p, [(b"nope", 1, 2, b"x")]) == view(p)
    assert both(p, []) == view(p)


def test_links_follow_chops_rule():
    p = fo.parse_gfa(A)
    q = im.inject(p, [(b"p", 5, 9, b"x"), (b"p", 1, 2, b"y")], links=True)
    # 1 is cut at 1 and 2: A, A, AA; 2 at 1: C, C; 3 whole
    assert view(q)[0] == ["A", "A", "AA", "C", "C", "GGG"]
    got = [(int(l["from_"]), int(l["to"])) for l in q.links]
    fwd = [(0 << 1, 1 << 1), (1 << 1, 2 << 1), (3 << 1, 4 << 1)]  # inside each cut segment
    old = [(2 << 1, (4 << 1) | 1), ((3 << 1) | 1, 5 << 1)]  # 1+ -> 2-: last piece of 1, last piece of 2; 2- -> 3+: first piece of 2
    assert got == fwd + old


REFUSED = {
    "a new name is a path of the graph": [(b"p", 1, 5, b"q")],
    "a new name twice": [(b"p", 1, 5, b"x"), (b"q", 0, 3, b"x")],
    "a line on an injected path": [(b"p", 4, 9, b"x"), (b"x", 1, 2, b"y")],
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_cases(what):
    p = fo.parse_gfa(A)
    lines = REFUSED[what]
    with pytest.raises(im.Refused) as e:
        im.inject(p, lines)
    assert e.value.line == len(lines) - 1
    _segs, paths = view(im.inject_sequential(p, lines))  # what the reference gives
    if what == "a new name is a path of the graph":
        assert list(paths) == ["p", "q"] and paths["q"] == ["2+", "4-"]  # q is replaced where it stands
    elif what == "a new name twice":
        assert paths["x"] == ["5-"]  # the later line wins: q's 3-, now segment 5
    else:
        assert paths["x"] == ["3-", "2-", "4+"] and paths["y"] == ["2-"]  # the injected path is found and cut
