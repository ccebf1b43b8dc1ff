"""Every planted graph of tests/extract_shapes.py gives, on the model, the answer derived by hand, and really exercises the
rule it is aimed at: the answer changes under the model variant (or the other arguments) the shape names."""
import pytest

import extract_model as em
from extract_shapes import SHAPES


def run(sh, variant=None, **over):
    a = {"n": sh.n, "c": sh.c, "d": sh.d, "e": sh.e, **over}
    return em.extract_by_name(sh.pools(), a["n"], a["c"], a["d"], a["e"], variant)


@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: s.name)
def test_shape_answer_by_hand(sh):
    q = run(sh)
    assert [int(x) for x in q.segs["name"]] == sh.segs, sh.rule
    assert [q.path_name(i) for i in range(len(q.paths))] == sh.paths, sh.rule
    assert len(q.line_order) == 0 and q.header.tobytes() == sh.pools().header.tobytes()


@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: s.name)
def test_shape_exercises_its_rule(sh):
    assert (sh.variant is None) != (sh.other is None), "a shape names exactly one proof"
    base = em.text(run(sh))
    changed = run(sh, sh.variant) if sh.variant else run(sh, **sh.other)
    assert em.text(changed) != base, sh.rule


def test_every_variant_is_used():
    assert {s.variant for s in SHAPES if s.variant} == em.VARIANTS
