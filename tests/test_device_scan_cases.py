"""The cases of tests/device_scan_cases.py, checked on the CPU: that the references would notice what they are there to
notice, that the inputs stay inside what device_scan.hpp promises to handle, and that the constants restated in Python are
those of tests/device_check/scan_check.hip."""
import os
import re

import numpy as np
import pytest

import device_scan_cases as dc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "device_check", "scan_check.hip")
BY_KIND = {k: [c for c in dc.CASES if c.kind == k] for k in {c.kind for c in dc.CASES}}


def test_ids_are_unique_and_every_kind_and_size_is_there():
    assert len({c.id for c in dc.CASES}) == len(dc.CASES)
    assert set(BY_KIND) == {"sum32", "sum64", "affine", "block_excl", "wave", "last_start", "check_links", "blocks"}
    for point in dc.POINTS:
        for kind in ("sum32", "sum64", "affine"):
            assert sorted({c.n for c in BY_KIND[kind] if c.point == dc.point_name(point)}) == sorted(set(dc.sizes(point)))
    assert max(c.n for c in dc.CASES) == 2 * 1024 * 2048 + 1 <= dc.MAX_N


def test_sizes_are_the_tile_arithmetic():
    assert dc.sizes((256, 4)) == [0, 1, 3, 4, 1023, 1024, 1025, 2051, 262143, 262144, 262145, 524289]
    assert dc.sizes((64, 1)) == [0, 1, 63, 64, 65, 131, 4095, 4096, 4097, 8193]
    for kt, kp in dc.POINTS:
        t = dc.tile((kt, kp))
        s = dc.sizes((kt, kp))
        assert t == kt * kp and {t - 1, t, t + 1, 2 * t + 3, kt * t - 1, kt * t, kt * t + 1, 2 * kt * t + 1, kp, 0, 1} <= set(s)
        # in tiles: one short of a spine round, exactly one, one past it, and past two
        assert [-(-n // t) for n in s[-4:]] == [kt, kt, kt + 1, 2 * kt + 1]


def test_constants_are_the_programs():
    text = open(SRC).read()
    assert int(re.search(r"kGuardByte = (0x[0-9A-Fa-f]+);", text).group(1), 16) == dc.GUARD_BYTE
    assert int(re.search(r"kMaxN = 1ull << (\d+);", text).group(1)) == dc.MAX_N.bit_length() - 1
    assert int(re.search(r"kWaveThreads = (\d+);", text).group(1)) == dc.WAVE_THREADS
    for kt, kp in dc.POINTS:
        assert 'point == "%dx%d") tiled_kind<%d, %d>' % (kt, kp, kt, kp) in text
    for t in dc.BLOCK_THREADS:
        assert "threads == %d) block_excl<T, %d>" % (t, t) in text
    assert text.count("Guarded<uint32_t> pstart(m, 0, st), out(n, %d, st)" % dc.SMALL_GUARD) == 1
    assert text.count("flags(1, %d, st)" % dc.SMALL_GUARD) == 1


@pytest.mark.parametrize("case", BY_KIND["sum32"], ids=lambda c: c.id)
def test_sum32_tiles_stay_below_32_bits_at_every_point(case):
    a = case.arrays().astype(np.uint64)
    for point in dc.POINTS:
        t = dc.tile(point)
        padded = np.concatenate([a, np.zeros(-len(a) % t, np.uint64)])
        assert len(a) == 0 or int(padded.reshape(-1, t).sum(axis=1).max()) < 1 << 32, point


def test_sum32_has_totals_past_32_bits_with_truncated_prefixes():
    for point in dc.POINTS:
        big = [c for c in BY_KIND["sum32"] if c.point == dc.point_name(point) and c.name == "big"]
        assert len(big) == 4
        for c in big:
            a = c.arrays()
            want, total = dc.sum32_reference(a)
            assert total == sum(int(x) for x in a[:5000]) + int(a[5000:].astype(np.uint64).sum())
            if c.n > point[0] * dc.tile(point):
                assert total > 1 << 32 and int(want[-1]) == (total - int(a[-1])) & dc.M32 != total - int(a[-1])


@pytest.mark.parametrize("case", BY_KIND["affine"], ids=lambda c: c.id)
def test_affine_reference_is_order_sensitive(case):
    """Every a is odd, so every element has an inverse mod 2^64 and composing with a fixed front and a fixed back loses
    nothing: reversing elements i and i + 1 changes the total, and the carry behind the pair, exactly when the two do not
    commute.  That is checked for every adjacent pair of every input; on the inputs small enough the sequential reference
    is run on reversed pairs as well."""
    ab = case.arrays()
    n = len(ab)
    assert (ab[:, 0] & np.uint64(1)).all()
    if n < 2:
        return
    assert (dc.affine_then(ab[:-1], ab[1:]) != dc.affine_then(ab[1:], ab[:-1])).any(axis=1).all()
    if n > dc.AFFINE_BY_HAND:
        return
    carries, total = dc.affine_reference(ab)
    got = np.array(carries, np.uint64).reshape(n, 2)
    assert dc.affine_step_errors(ab, got, np.array(total, np.uint64)) == []
    rng = np.random.default_rng(n)
    for i in {0, n - 2, int(rng.integers(0, n - 1))}:
        sw = ab.copy()
        sw[[i, i + 1]] = sw[[i + 1, i]]
        c2, t2 = dc.affine_reference(sw)
        assert t2 != total and c2[:i + 1] == carries[:i + 1]
        assert all(x != y for x, y in zip(c2[i + 2:], carries[i + 2:]))  # (every carry behind the pair)
        assert dc.affine_step_errors(sw, got, np.array(total, np.uint64)) != []


def test_affine_stepwise_check_sees_a_dropped_a_doubled_and_a_misplaced_element():
    ab = dc.affine_input(3000, 3)
    carries, total = dc.affine_reference(ab)
    good, total = np.array(carries, np.uint64).reshape(-1, 2), np.array(total, np.uint64)
    assert dc.affine_step_errors(ab, good, total) == []
    for i in (0, 1, 1024, 2999):
        for col in (0, 1):
            bad = good.copy()
            bad[i, col] += np.uint64(1)
            assert dc.affine_step_errors(ab, bad, total)[0] == i
    shifted = np.concatenate([good[:1], good[:-1]])  # (every carry one element late)
    assert dc.affine_step_errors(ab, shifted, total)[0] == 1
    assert dc.affine_step_errors(ab, good, total + np.uint64(1)) == [3000]


def test_small_references_on_hand_made_outputs():
    # block_excl: two lanes' worth of wrap, by hand
    v = np.array([0xFFFFFFFF, 2] * 64, np.uint32)
    out = np.concatenate([np.array([0, 0xFFFFFFFF] * 32, np.uint32) + np.repeat(np.arange(32, dtype=np.uint32), 2),
                          np.array([0, 0xFFFFFFFF] * 32, np.uint32) + np.repeat(np.arange(32, dtype=np.uint32), 2),
                          np.full(128, 32, np.uint32), np.full(64, 0xA5A5A5A5, np.uint32)]).tobytes()
    dc.check_block_excl(32, 64, v, out)
    with pytest.raises(AssertionError, match="guard"):
        dc.check_block_excl(32, 64, v, out[:-1] + b"\0")
    # last_start: the reference names the last of a run of equal starts
    ps, lo, hi, q = dc.last_start_table("top")
    want = dict(zip(q.tolist(), (np.searchsorted(ps[lo:hi + 1], q, side="right") - 1 + lo).tolist()))
    assert want[5] == 2 and want[4] == 0 and want[dc.M32] == 6 and want[dc.M32 - 1] == 4 and want[dc.M32 - 2] == 3 and want[1 << 40] == 6
    for name in ("whole", "inner", "one", "first", "pair"):
        ps, lo, hi, q = dc.last_start_table(name)
        assert (np.diff(ps.astype(np.int64)) >= 0).all() and (np.diff(ps.astype(np.int64)) == 0).sum() > 100
        assert lo <= hi < len(ps) and (q >= ps[lo]).all()
    # check_links: exactly the planted end is out of range
    for c in BY_KIND["check_links"]:
        head, lk = c.arrays()
        assert int(((lk[:, :2] >> 1) >= head[0]).sum()) == (0 if c.name == "clean" else 1)
        assert int(((lk[:, :2] >> 1) == head[0] - 1).sum()) > 100 and head[1] not in (0, 1) and not head[1] & head[2]
