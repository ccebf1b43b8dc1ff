"""tests/inject_shapes.py on the CPU: the vectorized form of the model equals the rule-by-rule one (tests/inject_model.py) on
seeded random images and on every shape of the GPU geometry tests that the slow form can answer in seconds; the large shapes
are the same generators at a larger argument.  fast_pools, which answers with every pool of the result, is pinned to
inject_model.inject(links=True) on images with links and seq spans of every kind, and the two spelling properties that the
GPU tests assert without the model are shown to hold of the model.  No GPU."""
import numpy as np
import pytest

import inject_model as m
import inject_shapes as sh
from oracle import flatgfa_oracle as fo


def test_fast_form_on_random_images():
    rng = np.random.default_rng(77)
    cuts = 0
    for _ in range(300):
        im = sh.random_image(rng, int(rng.integers(1, 9)), int(rng.integers(1, 5)), 10, int(rng.integers(0, 9)))
        a, b = sh.fast(im), sh.slow(im)
        assert sh.same(a, b), im
        cuts += len(a.seg_len) > len(im.seg_len)
    assert cuts > 100


SHAPES = {
    "seam ends": lambda: sh.seam_ends(2),
    "cut rows": sh.cut_rows,
    "257 segments": lambda: sh.many_segments(257),
    "4097 segments": lambda: sh.many_segments(4097),
    "expansion 6143": lambda: sh.expansion(sh.OUT_TILE * 3 - 1),
    "whole tiles backward": sh.whole_tiles_backward,
    "overlapping spans": sh.overlapping_spans,
    "long and short lines": lambda: sh.long_and_short_lines(5000),
    "many lines on one path": lambda: sh.many_lines_one_path(400),
    "unsorted, nested": sh.unsorted_nested,
    "257 lines": lambda: sh.line_counts(257),
    "1025 lines": lambda: sh.line_counts(1025),
}


@pytest.mark.parametrize("what", list(SHAPES))
def test_fast_form_on_the_shapes(what):
    im = SHAPES[what]()
    assert sh.same(sh.fast(im), sh.slow(im))


# ---- every pool ----
def dressed(rng, im: sh.Image) -> sh.Image:
    """Links of all four orientation pairs, self-loops on a cut segment and duplicates; seq spans anywhere in a short seq_data
    (aliased, backwards, with gaps); names of several lengths."""
    im = sh.scattered_spans(sh.with_links(im, int(rng.integers(0, 30)), seed=int(rng.integers(1 << 30))), seed=int(rng.integers(1 << 30)))
    if rng.random() < 0.5:
        im.names = [b"new" + b"x" * int(rng.integers(0, 4)) + b"%d" % i for i in range(len(im.line_path))]
    return im


def test_fast_pools_and_spelling_on_random_images():
    rng = np.random.default_rng(78)
    loops = cut_links = lines = 0
    for _ in range(300):
        im = dressed(rng, sh.random_image(rng, int(rng.integers(1, 9)), int(rng.integers(1, 5)), 10, int(rng.integers(0, 9))))
        p = sh.pools_of(im)
        want = m.inject(p, sh.lines_of(im), links=True)
        assert sh.differing(sh.fast_pools(im, links=True), want) == [], im
        assert sh.differing(sh.fast_pools(im), m.inject(p, sh.lines_of(im))) == [], im
        # spell_pool is spell, and the two properties hold of the model
        sp = sh.spell_pool(want)
        assert all(sh.spelled(sp, want, i) == sh.spell(want, i) for i in range(len(want.paths)))
        sh.check_spelling(im, p, want, sp)
        k = np.diff(sh.fast(im).seg_first) - 1
        f, t = im.links[:, 0], im.links[:, 1]
        loops += int(((f >> 1 == t >> 1) & (k[f >> 1] > 0)).sum())
        cut_links += int(((k[f >> 1] > 0) & (k[t >> 1] > 0)).sum())
        lines += len(im.lo)
    assert loops > 50 and cut_links > 300 and lines > 1000


NEW_SHAPES = {
    "60 long rows": lambda: sh.long_rows(60),
    "row lengths, short": lambda: sh.row_lengths((31, 32, 33, 17, 64)),
    "1023 segments": lambda: sh.many_segments(1023),
    "1025 segments": lambda: sh.many_segments(1025),
    "1023 pool steps": lambda: sh.pool_steps(1023),
    "1024 pool steps": lambda: sh.pool_steps(1024),
    "many paths, non tiling": sh.many_paths_non_tiling,
    "a ring": lambda: sh.ring(40, 60),
}


@pytest.mark.parametrize("what", list(SHAPES) + list(NEW_SHAPES))
def test_fast_pools_on_the_shapes(what):
    im = {**SHAPES, **NEW_SHAPES}[what]()
    if im.links is None:
        im = sh.with_links(im, 300, seed=1)
    if what in ("cut rows", "unsorted, nested", "60 long rows"):
        im = sh.scattered_spans(im, seed=2)
    p = sh.pools_of(im)
    assert sh.differing(sh.fast_pools(im, links=True), m.inject(p, sh.lines_of(im), links=True)) == []


def test_shapes_are_what_they_say():
    a = sh.fast(sh.cut_rows())
    k = np.diff(a.seg_first) - 1
    assert k.tolist() == [0, 1, 16, 17, 4097, 1, 2, 1]
    for t in (sh.OUT_TILE * 3 - 1, sh.OUT_TILE * 3, sh.OUT_TILE * 3 + 1):
        im = sh.expansion(t)
        a = sh.fast(im)
        assert a.path_end[0] == t and len(a.steps) == t  # (its lines are empty ones)
    a = sh.fast(sh.whole_tiles_backward())
    assert a.path_end[0] == 4100 and (a.steps[1:4099] & 1).all()
    im = sh.long_and_short_lines(5000)
    a = sh.fast(im)
    lens = (a.path_end - a.path_begin).tolist()
    assert lens[2:7] == [0, lens[0], 1, 3, 0] and lens[0] > 5000 and lens[7] > 0 and a.path_end[-1] == len(a.steps)
    im = sh.seam_ends(2)
    assert im.path_begin[1] == 7 and len(im.steps) == 7 + 2 * sh.TILE + 40
    # k_sort_long's rounds: R rows of more than LINEAR raw keys, a few of them with repeats
    for R in (sh.MAX_GRID, sh.MAX_GRID + 1, 2 * sh.MAX_GRID + 1):
        im = sh.long_rows(R)
        raw = sh.raw_rows(im)
        assert int((raw > sh.LINEAR).sum()) == R == len(raw) and raw.max() == 23 and (np.diff(sh.fast(im).seg_first) == 18).all()
        assert np.all(np.diff(im.lo[23:40]) < 0)  # (row 1, behind row 0's 23 lines: given in descending order)
    im = sh.row_lengths()
    assert sh.raw_rows(im).tolist() == list(sh.ROW_LENGTHS)
    k = (np.diff(sh.fast(im).seg_first) - 1).tolist()
    assert [a - b for a, b in zip(sh.ROW_LENGTHS, k)] == [4, 0, 0, 36, 0, 0, 73, 0, 0, 146]
    # k_sort_short's rounds, and the S + 1 scan on its tile seam
    one_round = sh.MAX_GRID * 256
    for S in (sh.SCAN_TILE - 1, sh.SCAN_TILE, sh.SCAN_TILE + 1, one_round, one_round + 1):
        im = sh.many_segments(S)
        raw = sh.raw_rows(im)
        assert len(raw) == S and raw[-1] >= 2 and raw.max() <= sh.LINEAR
        if S >= one_round:
            assert raw[one_round - 2:].tolist() == [5, 5 + 2 * (S == one_round), 7][:S - one_round + 2]
            rows = im.lo[-5 * (S - one_round + 2):].reshape(-1, 5)
            assert np.all(np.diff(rows, axis=1) < 0)
    # pre[N] and noff[N] at the scan tile's seam
    for N in (sh.SCAN_TILE - 2, sh.SCAN_TILE - 1, sh.SCAN_TILE):
        im = sh.pool_steps(N)
        a = sh.fast(im)
        assert len(im.steps) == N and im.path_end[-1] == N and im.path_begin[1] == im.path_end[0]
        total = 3 * (N - 300)
        assert (im.lo[:5].tolist(), im.hi[:5].tolist()) == ([total - 2, total - 5, total - 4, total - 1, total], [total - 1, total - 3, total, total + 1, total + 1])
        assert np.diff(a.seg_first)[im.steps[-1] >> 1] >= 3  # the last step of the pool is cut at both of its inner positions
    for n in (511, 512):
        assert 2 * n + 1 in (sh.SCAN_TILE - 1, sh.SCAN_TILE + 1)
    im = sh.many_paths_non_tiling()
    assert len(im.path_begin) == 4100 and len(im.steps) == 5000 and set(im.line_path.tolist()) == {0, 4095, 4096, 4099}
    assert not np.array_equal(im.path_begin[1:], im.path_end[:-1])
    a = sh.fast(im)
    assert all(a.path_end[p] - a.path_begin[p] > im.path_end[p] - im.path_begin[p] for p in (0, 4095, 4096, 4099))  # each is cut
