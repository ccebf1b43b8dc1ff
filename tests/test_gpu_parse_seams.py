"""The device GFA parser's verdict -- plain, or whose fault it is -- where a byte's predecessor lies in another lane, another
workgroup's tile or another 64-byte step of a wave: faults across those seams, fields of exactly the lengths the wave's steps
turn at, the text's end at every length mod 16, the first of grammar, limit and name found by different kernels in different
tiles, and the item limit on every total it is held against.  The oracle is the host parser on the same bytes in both modes
(test_gpu_parse.check_against_host: all eleven pools or the error sentence, and the route and reason of the regex model of
tests/parse_shapes.py); tests/test_parse_shapes.py pins every builder and class table on the host.  T is the tile size the
library reports, never a number written here.  Run with -m gpu."""
import numpy as np
import pytest

import pollen_amd as pa
import parse_shapes as ps
from test_gpu_parse import check_against_host

pytestmark = pytest.mark.gpu

MODES = (False, True)
ROUTE = {("plain", "accepts"): "device", ("limit", "accepts"): "host", ("grammar", "accepts"): "host",
         ("grammar", "error"): "error", ("name", "error"): "error"}


@pytest.fixture(scope="module")
def T():
    with pa.parse_bytes_device(b"S\t1\tA\n") as g:
        assert g.parsed_on == "device" and g.parse_info["tiles"] == 1
        return g.parse_info["tile_bytes"]


def run(text, stream, why=None):
    """check_against_host, with the reason the case was built for."""
    if why is not None:
        assert ps.reason(text, stream) == why
    return check_against_host(text, stream)


# ---- a fault on a step seam ----

def edge_cases(T, item, tail):
    """(x, k, text): the item's byte k on a tile's first byte and on a lane's first byte inside a tile."""
    for x in (T, T + ps.LANE):
        for k in range(-1, len(item) + 1):
            yield x, k, (ps.on_edge(T, x, k, item, tail) if tail else ps.on_edge(T, x, k, item))


@pytest.mark.parametrize("item", list(ps.STEP_ITEMS), ids=repr)
def test_step_item_across_a_lane_or_tile_edge(T, item):
    why, host = ps.STEP_ITEMS[item]
    for x, k, text in edge_cases(T, item, None):
        for stream in MODES:
            assert run(text, stream, why) == ROUTE[why, host], (x, k, stream)


@pytest.mark.parametrize("item", list(ps.FIELD_ENDS), ids=repr)
def test_field_end_across_a_lane_or_tile_edge(T, item):
    why, host = ps.FIELD_ENDS[item]
    for x, k, text in edge_cases(T, item, ps.FIELD_END_TAIL):
        for stream in MODES:
            assert run(text, stream, why) == ROUTE[why, host], (x, k, stream)


# ---- field lengths on the wave's steps ----

def test_field_ladder():
    text = ps.field_ladder()
    for stream in MODES:
        assert check_against_host(text, stream, "device") == "device"
        with pa.parse_bytes_device(text, stream) as g:
            assert g.parsed_on == "device"
            segs, paths, links = g.pool("segs"), g.pool("paths"), g.pool("links")
            assert sorted(set((segs["seq_end"] - segs["seq_start"]).tolist())) == list(ps.LADDER)
            assert sorted(set((segs["opt_end"] - segs["opt_start"]).tolist())) == list(ps.LADDER)
            assert set((paths["name_end"] - paths["name_start"]).tolist()) >= set(ps.LADDER)
            assert len(set((links["ov_end"] - links["ov_start"]).tolist())) > 40  # (ops, not bytes: 0 to 130 bytes of them)
            steps = (paths["steps_end"] - paths["steps_start"]).tolist()
            assert 0 in steps and max(steps) > 20  # the stretches: no steps, and 60 bytes and more of them


# ---- a fault on a wave seam ----

CIGARS = ps.cigar_family()


@pytest.mark.parametrize("name", list(CIGARS))
def test_cigar_fault(name):
    routes = [run(CIGARS[name], stream) for stream in MODES]
    assert routes[0] == routes[1]


def test_cigar_faults_come_by_every_route():
    count = {"device": 0, "host": 0, "error": 0}
    for text in CIGARS.values():
        count[check_against_host(text, False)] += 1
    assert min(count.values()) >= 10, count


# ---- the line index and the text's end ----

@pytest.mark.parametrize("name", ["kind X at byte T - 1", "kind X at byte T", "no tab at byte T", "an empty line across T", "a second header at T",
                                  "the one header at T"])
def test_line_index_on_a_tile_edge(T, name):
    text = ps.line_index_texts(T)[name]
    for stream in MODES:
        route = run(text, stream, "plain" if name == "the one header at T" else "grammar")
        assert (route == "device") == (name == "the one header at T")


@pytest.mark.parametrize("r", range(16))
def test_text_ends_r_bytes_into_a_lane(T, r):
    whole, broken = ps.unterminated(T, r, False), ps.unterminated(T, r, True)
    assert len(whole) == T + ps.LANE + r and whole.count(b"\nP\t") == 1 and not whole.endswith(b"\n")
    for text in (whole, broken):  # parse_mem never sees the last line
        assert run(text, False, "plain") == "device"
        with pa.parse_bytes_device(text) as g:
            assert (g.parsed_on, g.path_count) == ("device", 0)
    assert run(whole, True, "plain") == "device"
    with pa.parse_bytes_device(whole, stream=True) as g:
        assert (g.parsed_on, g.path_count) == ("device", 1)
        assert g.pool("steps").tolist() == [0 << 1, 1 << 1 | 1]
    assert run(broken, True, "grammar") in ("host", "error")  # the virtual last line is an invalid one


@pytest.mark.parametrize("kind", ["S", "P", "L", "H"])
def test_kind_byte_is_the_last_byte(T, kind):
    text = ps.lone_kind(T, kind.encode())
    assert run(text, False, "plain") == "device"
    assert run(text, True, "grammar") in ("host", "error")


# ---- the first of grammar, limit and name ----

PAIRS, TRIPLES = ps.precedence_pairs(), ps.precedence_triples()


@pytest.mark.parametrize("name", list(PAIRS))
def test_precedence_of_two_faults(T, name):
    ca, la, cb, lb = PAIRS[name]
    first = min(ca, cb, key=ps.PRECEDENCE.index)
    for text in ps.pair_texts(T, list(PAIRS).index(name), la, lb):
        for stream in MODES:
            assert run(text, stream, first) in ("host", "error")
            assert pa.parse_device_info()["reason"] == first


@pytest.mark.parametrize("name", list(TRIPLES))
def test_precedence_of_three_faults(T, name):
    for text in ps.triple_texts(T, *TRIPLES[name]):
        for stream in MODES:
            assert run(text, stream, "grammar") in ("host", "error")
            assert pa.parse_device_info()["reason"] == "grammar"


@pytest.mark.parametrize("cls", list(ps.FAULTS))
def test_every_fault_alone(T, cls):
    for k, line in enumerate(ps.FAULTS[cls].values()):
        for t in range(3):
            for stream in MODES:
                assert run(ps.faults_in_tiles(T, {t: line}), stream, cls) in ("host", "error")
                assert pa.parse_device_info()["reason"] == cls
    assert run(ps.faults_in_tiles(T, {}), False, "plain") == "device"


# ---- small texts ----

SMALL = ps.small_texts()


@pytest.mark.parametrize("first", ["S", "\t", "1", "\n"], ids=["S", "tab", "1", "newline"])
def test_small_texts(first):
    """Every text of at most five bytes over S, tab, 1 and newline, by its first byte (the empty text goes with the last)."""
    texts = [t for t in SMALL if t[:1] == first.encode() or (not t and first == "\n")]
    assert len(texts) == 341 + (first == "\n")
    for text in texts:
        for stream in MODES:
            check_against_host(text, stream)


def test_small_texts_take_the_device_route():
    n = sum(ps.plain(t, s) for t in SMALL for s in MODES)
    assert n == 372
    on_device = 0
    for text in SMALL:
        for stream in MODES:
            if ps.plain(text, stream):
                with pa.parse_bytes_device(text, stream) as g:
                    on_device += g.parsed_on == "device"
    assert on_device >= 300 and on_device == n


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_prefixes_of_a_handmade_text(name):
    text = ps.HANDMADE[name]
    routes = {check_against_host(text[:n], stream) for n in range(len(text)) for stream in MODES}
    assert "device" in routes


# ---- the item limit ----

@pytest.mark.parametrize("what", list(ps.LIMIT_TEXTS))
def test_item_limit(monkeypatch, what):
    """The hook at the text's one largest quantity: the device route; at one less: the host route, for "limit", and the same
    pools.  (Segments, paths and links are never more than the lines, and overlaps never more than ops: see LIMIT_TEXTS.)"""
    text = ps.LIMIT_TEXTS[what]
    for stream in MODES:
        with (pa.parse_stream_bytes if stream else pa.parse_bytes)(text) as h:
            want = ps.pools_of(h)
        q = ps.quantities(want)
        assert q[what] == max(q.values())
        monkeypatch.setenv("FLATGFA_PARSE_DEVICE_LIMIT", str(q[what]))
        with pa.parse_bytes_device(text, stream) as g:
            assert (g.parsed_on, g.parse_reason) == ("device", "plain")
            assert ps.pools_of(g) == want
        monkeypatch.setenv("FLATGFA_PARSE_DEVICE_LIMIT", str(q[what] - 1))
        with pa.parse_bytes_device(text, stream) as g:
            assert (g.parsed_on, g.parse_reason) == ("host", "limit")
            assert ps.pools_of(g) == want
        monkeypatch.delenv("FLATGFA_PARSE_DEVICE_LIMIT")
        with pa.parse_bytes_device(text, stream) as g:
            assert (g.parsed_on, g.parse_reason) == ("device", "plain")
