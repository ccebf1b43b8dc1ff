"""tests/print_model.py, the restatement of print.rs that the device printer's tests compare with, equals the host printer
(FlatGFA.gfa_text) on every golden graph and on handmade texts that use each of its rules.  No GPU."""
import pytest

import pollen_amd as pa
import print_model as pm
import print_shapes as ps
from conftest import fixture_id, golden_gfas


def read(path):
    with open(path, "rb") as f:
        return f.read()


def load(p, tmp_path):
    f = tmp_path / "shape.flatgfa"
    f.write_bytes(ps.fo.dump_flatgfa(p))
    return pa.load(str(f))


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_golden(gfa):
    with pa.parse_bytes(read(gfa)) as g:
        assert pm.gfa(pm.pools_of(g)) == g.gfa_text()


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade(name):
    text = ps.HANDMADE[name]
    with pa.parse_bytes(text) as g:
        got = pm.gfa(pm.pools_of(g))
        assert got == g.gfa_text()
        if text.endswith(b"\n") and name not in ("CIGARs of several ops", "path overlaps"):
            assert got == text  # the printer gives these texts back as they are (but D and I change places: print.rs:18-19)


def test_handmade_texts_use_the_rules():
    with pa.parse_bytes(ps.HANDMADE["header in the middle"]) as g:
        assert g.pool("line_order").tolist() == [pm.S, pm.S, pm.H, pm.L, pm.P]
    with pa.parse_bytes(ps.HANDMADE["P before S"]) as g:
        assert g.pool("line_order").tolist()[0] == pm.P
    with pa.parse_bytes(ps.HANDMADE["CIGARs of several ops"]) as g:
        assert len(g.pool("alignment")) == 4 + 1 + 2
    with pa.parse_bytes(ps.HANDMADE["path overlaps"]) as g:
        assert len(g.pool("overlaps")) == 3
    with pa.parse_bytes(ps.HANDMADE["a 20-digit name"]) as g:
        assert int(g.pool("segs")["name"].max()) == ps.U64_MAX


@pytest.mark.parametrize("make", [ps.digit_names, lambda: ps.alternating(40), lambda: ps.long_overlaps(50),
                                  lambda: ps.long_cigar(30, 10), lambda: ps.path_name(65)],
                         ids=["digit names", "alternating", "long overlaps", "long cigar", "path name"])
def test_builders(make):
    text = make()
    with pa.parse_bytes(text) as g:
        assert pm.gfa(pm.pools_of(g)) == g.gfa_text()
        assert len(g.gfa_text()) == len(text)


def test_pools_no_text_gives(tmp_path):
    text = ps.alternating(12)
    for p in (ps.short_line_order(text, 7), ps.normalized(text), ps.shared_steps(text), ps.normalized(ps.HANDMADE["P before S"]),
              ps.wide_ops(ps.long_cigar(30, 10)), ps.wide_ops(ps.HANDMADE["path overlaps"])):
        with load(p, tmp_path) as g:
            assert pm.gfa(p) == g.gfa_text()
    with load(ps.short_line_order(text, 7), tmp_path) as g:
        assert g.gfa_text() == b"".join(text.splitlines(True)[:7])


ERRORS = {
    "print: empty header": lambda: ps.with_pools(ps.fo.parse_gfa(ps.HANDMADE["plain"]), header=ps.np.zeros(0, ps.np.uint8)),
    "print: too few segments": lambda: ps.order_of(ps.HANDMADE["plain"], [0, 1, 1, 1, 2, 1, 3]),
    "print: too few paths": lambda: ps.order_of(ps.HANDMADE["plain"], [1, 2, 3, 2]),
    "print: too few links": lambda: ps.order_of(ps.HANDMADE["plain"], [3, 3, 3]),
    "print: bad line kind": lambda: ps.order_of(ps.HANDMADE["plain"], [1, 4]),
    "print: path with no steps": lambda: ps.path_without_steps(ps.HANDMADE["path overlaps"], 1),
}


@pytest.mark.parametrize("message", list(ERRORS))
def test_errors(message, tmp_path):
    p = ERRORS[message]()
    with pytest.raises(pm.PrintError, match=message):
        pm.gfa(p)
    with load(p, tmp_path) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            g.gfa_text()
        assert e.value.code == -2 and pa._lib.last_error() == message
