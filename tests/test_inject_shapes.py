"""tests/inject_shapes.py on the CPU: the vectorized form of the model equals the rule-by-rule one (tests/inject_model.py) on
seeded random images and on every shape of the GPU geometry tests that the slow form can answer in seconds; the large shapes
are the same generators at a larger argument.  No GPU."""
import numpy as np
import pytest

import inject_shapes as sh


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
