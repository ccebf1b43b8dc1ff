"""tests/bed_model.py, the yardstick of the BED intersect tests, pinned on cases whose output is written out by hand from
cli/cmds.rs:404-412 and flatbed.rs:37-57,125-158.  No device, no library."""
import random

import pytest

import bed_model as bm
import bed_shapes as bs

CASES = {
    "partial overlap reports the overlap only": (b"x\t10\t20\n", b"x\t15\t30\nx\t0\t12\n", b"x\t15\t20\nx\t10\t12\n"),
    "touching intervals give nothing": (b"x\t10\t20\n", b"x\t20\t30\nx\t0\t10\n", b""),
    "a inside x": (b"x\t10\t20\n", b"x\t0\t100\n", b"x\t10\t20\n"),
    "x inside a": (b"x\t0\t100\n", b"x\t10\t20\n", b"x\t10\t20\n"),
    "duplicates print twice": (b"x\t1\t5\nx\t1\t5\n", b"x\t2\t9\nx\t2\t9\n", b"x\t2\t5\n" * 4),
    "an empty name": (b"\t1\t5\nx\t1\t5\n", b"\t2\t9\n", b"\t2\t5\n"),
    "a # header line": (b"#name\tstart\tend\nx\t1\t5\n", b"#x\t0\t9\nx\t0\t9\n", b"x\t1\t5\n"),
    "an unterminated last line is dropped": (b"x\t1\t5\nx\t1\t7", b"x\t0\t9\nx\t0\t3", b"x\t1\t5\n"),
    "the largest number": (b"x\t5\t18446744073709551615\n", b"x\t0\t18446744073709551615\n", b"x\t5\t18446744073709551615\n"),
    "names differ": (b"x\t1\t5\n", b"y\t1\t5\nxx\t1\t5\nX\t1\t5\n", b""),
    "a's order outside, b's order inside": (b"x\t0\t9\ny\t0\t9\nx\t2\t3\n", b"y\t1\t2\nx\t2\t4\nx\t1\t3\n",
                                            b"x\t2\t4\nx\t1\t3\ny\t1\t2\nx\t2\t3\nx\t2\t3\n"),
    "columns after the third are ignored": (b"x\t1\t5\tgene\t+\n", b"x\t2\t9\t.\n", b"x\t2\t5\n"),
    "numbers wrap": (b"x\t18446744073709551617\t36893488147419103242\n", b"x\t0\t100\n", b"x\t1\t10\n"),
    "empty intervals print nothing": (b"x\t5\t5\nx\t9\t2\n", b"x\t0\t100\n", b""),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written(name):
    a, b, want = CASES[name]
    assert bm.intersect(a, b) == want


def test_parse_rules():
    assert bm.parse(b"\t1\t2\n#c\nlong name with spaces\t03\t4x\trest\n") == [(b"", 1, 2), (b"long name with spaces", 3, 4)]
    assert bm.parse(b"x\t1 2\n") == [(b"x", 1, 2)]  # (the byte behind the start column is not looked at)
    for bad, what in [(b"x\n", "expected number"), (b"\n", "expected number"), (b"x\tq\t2\n", "expected number"),
                      (b"x\t1\n", "line ends after the start column"), (b"x\t1\t\n", "expected number")]:
        with pytest.raises(bm.BedError, match=what):
            bm.parse(bad)


def test_pairs_carry_the_indices():
    a, b = bm.parse(b"x\t0\t9\ny\t0\t9\n"), bm.parse(b"y\t1\t2\nx\t2\t4\nx\t1\t3\n")
    assert bm.pairs(a, b) == [(0, 1, 2, 4), (0, 2, 1, 3), (1, 0, 1, 2)]
    ids, order = bm.grouped(b)
    assert ids == {b"y": 0, b"x": 1} and order == [0, 1, 2]
    ids, order = bm.grouped(bm.parse(b"p\t0\t1\nq\t0\t1\np\t5\t6\n"))
    assert order == [0, 2, 1]


def test_shapes_parse_and_are_not_trivial():
    hits = 0
    for name, (a, b) in bs.SHAPES.items():
        hits += bm.intersect(a, b).count(b"\n")
    assert hits > 30
    rng = random.Random(5)
    sizes = [bm.intersect(*bs.random_case(rng)).count(b"\n") for _ in range(40)]
    assert sum(1 for n in sizes if n) > 20 and 0 in sizes
