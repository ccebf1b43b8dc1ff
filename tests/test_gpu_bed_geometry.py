"""BED intersection at the seams of its layout -- tiles of candidates, rounds, the tiles of the group scan, the 16 KiB tiles and
4 MiB pieces of the text, the 64-byte cut between a lane's copy of a name and the workgroup's -- each at the smallest shape
that reaches it, against tests/bed_model.py byte for byte.  Run with -m gpu."""
import os
import random
import re

import pytest

import bed_model as bm
import bed_shapes as bs
import pollen_amd as pa
from conftest import ROOT
from test_gpu_bed import check, device_records

pytestmark = pytest.mark.gpu
CT, ST, TILE, PIECE, LONG = bs.CAND_TILE, bs.SCAN_TILE, bs.TILE, bs.PIECE, bs.LONG_NAME
CSRC = os.path.join(ROOT, "pollen_amd", "csrc")


def constant(header: str, name: str) -> int:
    src = open(os.path.join(CSRC, header)).read()
    expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
    return int(eval(re.sub(r"\(uint\d+_t\)", "", expr)))


def test_the_mirror_is_true():
    from pollen_amd import device
    assert constant("bed_device.hpp", "kBedThreads") == bs.THREADS
    assert constant("bed_device.hpp", "kBedCandTile") == CT
    assert constant("bed_device.hpp", "kBedThreads") * constant("bed_device.hpp", "kBedScanPer") == ST
    assert constant("bed_device.hpp", "kBedRoundCands") == bs.ROUND_CANDS == device.BED_ROUND_CANDS
    assert constant("flatten_device.hpp", "kFlatTile") == TILE
    assert constant("flatten_device.hpp", "kFlatPieceBytes") == PIECE
    assert constant("flatten_device.hpp", "kFlatLongName") == LONG


def counts(a, b):
    return pa.bed_intersect_count(a, b)


# ---- candidate tiles ----

@pytest.mark.parametrize("n", [CT - 1, CT, CT + 1, 2 * CT + 5, 3 * CT + 1])
def test_candidates_at_the_tile_edges(n):
    """One A entry over n sorted, disjoint B intervals: n candidates, all of them hits; from 2 tiles + 5 on one entry's
    candidates span more than two tiles."""
    a, b = b"x\t0\t%d\n" % (10 * n), bs.text(bs.run(b"x", n))
    want = check(a, b)
    assert counts(a, b) == (n, len(want), n, 0)
    got, pairs = device_records(a, b)
    assert got == pairs and len(got) == n


def test_entries_without_candidates_around_a_tiles_owner():
    """Runs of A entries that have no candidate -- other names, empty intervals, intervals in a gap of B -- in front of,
    between and behind the entries whose candidates a tile starts in; the second owner's candidates begin inside tile 0 and the
    third's exactly on tile 1."""
    b = bs.text(bs.run(b"x", 700, 10, 10))  # [0,10) [20,30) ...: gaps of 10
    none = [(b"y", 0, 99999), (b"x", 5, 5), (b"x", 10, 20), (b"x", 9, 3)]
    a = bs.text(none * 3 + [(b"x", 0, 20 * 600)] + none * 400 + [(b"x", 0, 20 * 424)] + none * 2 + [(b"x", 100, 20 * 700)] + none * 300)
    want = check(a, b)
    assert counts(a, b)[2] == 600 + 424 + 695 == want.count(b"\n")
    got, pairs = device_records(a, b)
    assert got == pairs


# ---- rounds ----

@pytest.mark.parametrize("round_cands", [1, 2, CT + 1, None])
def test_round_cuts(round_cands, monkeypatch):
    """The round cuts move, the text does not (FLATGFA_BED_ROUND_CANDS is a test hook).  x's group is unsorted, so every A
    entry of x meets all ten of its entries and hits the first and the last only: with rounds of 2, rounds without a hit lie
    between rounds that have one."""
    x = [(b"x", 0, 10)] + [(b"x", 500 + k, 501 + k) for k in (7, 3, 5, 1, 6, 2, 4, 0)] + [(b"x", 5, 20)]
    b = bs.text(x + bs.run(b"y", 40))
    a = bs.text([(b"x", 0, 100)] * 3 + [(b"y", 0, 10_000)] * (3 if round_cands in (1, 2) else 60))
    want = bm.intersect(a, b)
    if round_cands is not None:
        monkeypatch.setenv("FLATGFA_BED_ROUND_CANDS", str(round_cands))
    assert check(a, b) == want
    lines, _, cands, unsorted = counts(a, b)
    assert unsorted == 1 and cands == 3 * 10 + a.count(b"y") * 40 and lines == 3 * 2 + a.count(b"y") * 40
    if round_cands == 2:
        pieces = []
        pa.bed_intersect_stream(a, b, pieces.append)
        assert b"".join(pieces) == want and len(pieces) == 6 + 3 * 20  # a piece per round with a hit: rounds 0 and 4 of each five
        assert pieces[:2] == [b"x\t0\t10\n", b"x\t5\t20\n"]
    got, pairs = device_records(a, b, **({} if round_cands is None else {"round_cands": round_cands}))
    assert got == pairs


# ---- the scan over the groups ----

def sorted_disjoint(groups):
    """(a, b): B's groups of the given sizes, sorted and disjoint; A a short interval inside every eleventh B interval"""
    b = sum((bs.run(b"g%d" % k, n, 10, 10) for k, n in enumerate(groups)), [])
    a = [(nm, s + 2, s + 7) for nm, s, _ in b[::11]] + [(nm, s + 8, e + 12) for nm, s, e in b[5::97]]
    return bs.text(a), bs.text(b)


@pytest.mark.parametrize("groups", [[ST, ST - 1, 7], [1, ST - 1, ST], [2 * ST + 300, 5], [ST - 1, 1, 1, ST + 1]], ids=str)
def test_group_heads_at_the_scan_tile_edges(groups):
    """A group's head on the first and on the last element of a scan tile, a group longer than two tiles.  On sorted,
    disjoint, non-empty B with non-empty A the two bisections leave exactly the entries that overlap: candidates == lines."""
    a, b = sorted_disjoint(groups)
    want = check(a, b)
    lines, _, cands, unsorted = counts(a, b)
    assert lines == cands == want.count(b"\n") > 0 and unsorted == 0


def test_a_huge_end_does_not_leak_into_the_next_group():
    b = [(b"big", 0, bs.U64_MAX)] + bs.run(b"small", 50, 10, 10) + [(b"big2", 7, bs.U64_MAX - 1)] + bs.run(b"small2", ST + 3, 10, 10)
    a = [(b"small", 21, 29), (b"small2", 20 * (ST + 1) + 1, 20 * (ST + 1) + 2), (b"big", 5, 6), (b"small", 0, 10_000), (b"big2", 0, 8)]
    a, b = bs.text(a), bs.text(b)
    want = check(a, b)
    lines, _, cands, unsorted = counts(a, b)
    assert lines == cands == 1 + 1 + 1 + 50 + 1 == want.count(b"\n") and unsorted == 0


def test_nested_b_reaches_back_to_the_long_interval():
    a, b = bs.SHAPES["nested b"]
    assert check(a, b) == b"x\t500\t600\n"
    assert counts(a, b) == (1, 10, 3, 0)  # lo reaches index 0: [0,1000) and the two short ones behind it are tried
    got, _ = device_records(a, b)
    assert got == [(0, 0, 500, 600)]


def test_equal_starts_count_as_sorted():
    a, b = bs.SHAPES["equal starts"]
    assert check(a, b) == b"x\t6\t9\nx\t6\t8\nx\t6\t9\n"
    assert counts(a, b)[3] == 0


def test_one_descending_pair_unsorts_its_group_alone():
    left, right = bs.run(b"l", 30, 10, 10), bs.run(b"r", 30, 10, 10)
    mid = bs.run(b"m", 30, 10, 10)
    mid[17], mid[18] = mid[18], mid[17]
    a, b = bs.text([(b"l", 42, 47), (b"m", 42, 47), (b"r", 42, 47), (b"m", 0, 5)]), bs.text(left + mid + right)
    want = check(a, b)
    assert want == b"l\t42\t47\nm\t42\t47\nr\t42\t47\nm\t0\t5\n"
    assert counts(a, b) == (4, len(want), 1 + 30 + 1 + 30, 1)  # the neighbours stay pruned; m is walked whole


# ---- names ----

def test_interleaved_names_are_grouped_stably():
    """B's names alternate line by line and each group's file order is not its start order's reverse: the text keeps B's
    file order inside a name."""
    p = [(b"p", s, s + 50) for s in (40, 10, 30, 20, 0)]
    q = [(b"q", s, s + 50) for s in (0, 20, 10, 40, 30)]
    a, b = b"q\t0\t100\np\t0\t100\n", bs.text(bs.interleave(p, q))
    want = check(a, b)
    assert [ln.split(b"\t")[1] for ln in want.split(b"\n")[:-1]] == [b"0", b"20", b"10", b"40", b"30", b"40", b"10", b"30", b"20", b"0"]
    assert counts(a, b)[3] == 2


@pytest.mark.parametrize("n", [0, 1, LONG, LONG + 1, TILE + 100])
def test_name_lengths(n):
    """a lane's copy up to kFlatLongName bytes, the workgroup's past it, a name longer than a tile"""
    name = (b"contig-" * (n // 7 + 1))[:n]
    other = name + b"x"
    a = bs.text([(name, 0, 100), (other, 0, 100), (name, 3, 4)])
    b = bs.text([(other, 5, 6), (name, 1, 9), (b"only-b", 0, 100), (name, 0, 50)])
    want = check(a, b)
    assert want.count(b"\n") == 5


# ---- text ----

@pytest.mark.parametrize("first", [b"x\t5\t20\n", b"x\t10\t20\n", b"x\t10\t100\n"])
def test_lines_at_a_text_tile_edge(first):
    """Eight-byte lines behind a first line of 7, 8 or 9 bytes: a line ends one before, exactly at and one after every 16 KiB
    boundary."""
    n = 2 * TILE // 8 + 3
    s, e = first.split()[1:]
    a = b"x\t%s\t%s\n" % (s, e) + b"x\t10\t20\n" * (n - 1)
    b = b"x\t5\t200\n"
    want = check(a, b)
    assert want == first + b"x\t10\t20\n" * (n - 1)
    assert (TILE - len(first)) % 8 == {7: 1, 8: 0, 9: 7}[len(first)]


def test_two_pieces_travel():
    a = bs.text(bs.run(b"chr1", 300_000, 10, 0, at=1_000_000))
    b = b"chr1\t0\t999999999\n"
    want = bm.intersect(a, b)
    assert PIECE < len(want) < 2 * PIECE
    sizes = []
    pa.bed_intersect_stream(a, b, lambda p: sizes.append(len(p)))
    assert sizes == [PIECE, len(want) - PIECE]
    assert pa.bed_intersect(a, b) == want
    assert counts(a, b) == (300_000, len(want), 300_000, 0)


def test_one_and_twenty_digits_in_a_line():
    a = b"x\t5\t18446744073709551615\nx\t0\t7\n"
    b = b"x\t0\t18446744073709551615\nx\t10000000000000000000\t18446744073709551615\n"
    assert check(a, b) == b"x\t5\t18446744073709551615\nx\t10000000000000000000\t18446744073709551615\nx\t0\t7\n"


# ---- empties ----

@pytest.mark.parametrize("name", ["empty intervals", "empty a", "empty b", "both empty"])
def test_empties(name):
    a, b = bs.SHAPES[name]
    want = check(a, b)
    assert want == (b"x\t1\t2\n" if name == "empty intervals" else b"")
    if name != "empty intervals":
        assert counts(a, b) == (0, 0, 0, 0)


# ---- a seeded random differential slice ----

@pytest.mark.parametrize("seed", range(6))
def test_random_slice(seed):
    """50 cases a seed of at most 200 x 200 lines over at most 4 names, sorted and unsorted groups mixed; none is skipped."""
    rng = random.Random(1000 + seed)
    hits = unsorted = 0
    for _ in range(50):
        a, b = bs.random_case(rng)
        want = bm.intersect(a, b)
        assert pa.bed_intersect(a, b) == want
        lines, nbytes, cands, uns = counts(a, b)
        assert (lines, nbytes) == (want.count(b"\n"), len(want)) and cands >= lines
        hits += lines
        unsorted += uns
    assert hits > 1000 and unsorted > 10
