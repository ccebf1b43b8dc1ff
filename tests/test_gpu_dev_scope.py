"""The device scope every host route opens (DevScope in pollen_amd/csrc/capi.cpp: pangenotype, GAF lookup, chop, extract,
position, validate, degree), seen from outside on one tiny graph: a call that is refused gives back what it held (the
next call on the handle answers as the models do), a handle answers the same before and after it becomes resident, and
two hundred calls that take one and two streams in turn leave the stream pool sound.  Every refusal here is an error
return.  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import chop_model as cm
import extract_model as em
import gaf_lookup_model as M
import gaf_model as gm
import pollen_amd as pa
import topology_model as tm
from gaf_lookup_shapes import gaf_line
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_BOUNDS = -1, -2

# 8 segments, 3 paths, 6 links
GFA = (b"S\t1\tACGT\nS\t2\tAC\nS\t3\tGGA\nS\t4\tT\nS\t5\tCCCCA\nS\t6\tTG\nS\t7\tA\nS\t8\tGATTACA\n"
       b"P\tx\t1+,2+,3+,4+,5+\t*\nP\ty\t1+,3+,4-,6+,8+\t*\nP\tz\t7+,8-,2+\t*\n"
       b"L\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nL\t4\t+\t5\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t7\t+\t8\t-\t0M\n")
GOOD = gaf_line(b"a", b">1>2>3", 1, 7) + gaf_line(b"b", b"<8>2", 2, 8) + gaf_line(b"c", b">5", 0, 4) + gaf_line(b"d", b">6>8", 1, 5)
# the second of (at least) four chunks names a segment the graph lacks
BAD = gaf_line(b"a", b">1>2", 1, 5) + gaf_line(b"b", b">1>99", 0, 3) + gaf_line(b"c", b">5", 0, 4) + gaf_line(b"d", b">6", 0, 1)
BAD_AT = len(gaf_line(b"a", b">1>2", 1, 5))


@pytest.fixture(scope="module")
def model():
    g = pa.parse_bytes(GFA)
    p = cm.pools_of(g)
    g.close()
    assert (len(p.segs), len(p.paths), len(p.links)) == (8, 3, 6)
    names = [int(s["name"]) for s in p.segs]
    return {
        "pools": p,
        "matrix": gm.matrix([GOOD, GOOD[:len(GOOD) // 2]], names),
        "seqs": M.seqs_text(M.Graph.from_gfa(GFA), GOOD),
        "count": M.count(M.Graph.from_gfa(GFA), GOOD)[0],
        "chop": cm.chop(p, 2, True),
        "extract": em.extract_by_name(p, 3, 1),
        "position": em.position(p, 1, 6),
        "validate": tm.validate(p),
        "degree": tm.degree(p),
    }


def position_rc(g, path, offset):
    hd, off, found = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_int()
    rc = _lib.lib().flatgfa_position(g._h, path, offset, ctypes.byref(hd), ctypes.byref(off), ctypes.byref(found))
    return rc, ((hd.value, off.value) if found.value else None)


def extract_rc(g, origin, dist):
    h = ctypes.c_void_p()
    rc = _lib.lib().flatgfa_extract(g._h, origin, dist, 300000, 6, ctypes.byref(h))
    return rc, (pa.FlatGFA(h.value) if h.value else None)


def same_pools(q, want):
    got = cm.pools_of(q)
    return all(getattr(got, n).tobytes() == getattr(want, n).tobytes() for n in fo.POOL_ORDER)


def answers(g):
    """Every route once, as comparable values."""
    return {
        "matrix": g.pangenotype_matrix([GOOD, GOOD[:len(GOOD) // 2]]).tolist(),
        "seqs": g.gaf_seqs(GOOD),
        "count": g.gaf_count(GOOD),
        "chop": g.chop(2, links=True).gfa_text(),
        "extract": g.extract(3, 1).gfa_text(),
        "position": position_rc(g, 1, 6),
        "validate": g.validate().tobytes(),
        "degree": g.degree().tolist(),
    }


def assert_model(got, model):
    assert got["matrix"] == model["matrix"]
    assert got["seqs"] == model["seqs"] and got["count"] == model["count"]
    assert got["chop"] == cm.text(model["chop"])
    assert got["extract"] == em.text(model["extract"])
    assert got["position"] == (0, model["position"])
    assert got["validate"] == model["validate"].tobytes() and len(model["validate"]) > 0
    assert got["degree"] == model["degree"].tolist()


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_refusal_then_success_on_one_handle(model, monkeypatch, resident):
    g = pa.parse_bytes(GFA)
    if resident:
        g.to_device(0)
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", "1")  # a chunk per line
    # GAF lookup and pangenotype: the second chunk is refused while the third is on its way
    for call in (g.gaf_seqs, g.gaf_count, g.gaf_table):
        with pytest.raises(pa.FlatGFAError) as e:
            call(BAD)
        assert e.value.code == ERR_BOUNDS and f"byte offset {BAD_AT} " in str(e.value)
        assert g.gaf_seqs(GOOD) == model["seqs"] and g.gaf_count(GOOD) == model["count"]
    with pytest.raises(pa.FlatGFAError) as e:
        g.pangenotype_matrix([GOOD, BAD])
    assert e.value.code == ERR_BOUNDS and f"file 1: the line at byte offset {BAD_AT} " in str(e.value)
    assert g.pangenotype_matrix([GOOD, GOOD[:len(GOOD) // 2]]).tolist() == model["matrix"]
    # position: a path index out of range
    assert position_rc(g, 3, 0)[0] == ERR_BOUNDS
    assert position_rc(g, 1, 6) == (0, model["position"])
    # chop: max_size = 0
    with pytest.raises(pa.FlatGFAError) as e:
        g.chop(0, links=True)
    assert e.value.code == ERR_ARG
    assert same_pools(g.chop(2, links=True), model["chop"])
    # extract: an origin segment out of range, then a real extract
    rc, q = extract_rc(g, 8, 1)
    assert rc == ERR_BOUNDS and q is None
    rc, q = extract_rc(g, 2, 1)
    assert rc == 0 and same_pools(q, model["extract"])
    # a link that names a segment the graph lacks (the handle's own link pool, overwritten in place) is found on the device,
    # by chop, extract, validate and degree alike, with the route's uploads, job and stream in hand
    data, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, 3, ctypes.byref(data), ctypes.byref(n), None) == 0 and n.value == 6
    to = ctypes.c_uint32.from_address(data.value + 4)
    good = to.value
    to.value = 99 << 1
    try:
        for call in (lambda: g.chop(2, links=True), lambda: g.extract(3, 1), g.validate, g.degree):
            with pytest.raises(pa.FlatGFAError, match="link") as e:
                call()
            assert e.value.code == ERR_BOUNDS
    finally:
        to.value = good
    assert_model(answers(g), model)
    g.close()


def test_resident_and_host_handles_answer_alike(model, monkeypatch):
    g = pa.parse_bytes(GFA)
    host = answers(g)
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", "64")  # (several lines a chunk, several chunks)
    assert answers(g) == host
    monkeypatch.delenv("FLATGFA_GAF_CHUNK_BYTES")
    h2d, plan = ctypes.c_double(), ctypes.c_double()
    assert _lib.lib().flatgfa_residency_ms(g._h, ctypes.byref(h2d), ctypes.byref(plan)) != 0  # no route made it resident
    g.to_device(0)
    assert answers(g) == host
    assert_model(host, model)
    fresh = pa.parse_bytes(GFA)  # resident before any route ran
    fresh.to_device(0)
    assert answers(fresh) == host
    d, u = fresh.seg_depth_with_uniq()
    wd, wu = fo.seg_depth_with_uniq(model["pools"])
    assert np.array_equal(d, wd) and np.array_equal(u, wu)  # the image the routes read in place is as it was
    fresh.close()
    g.close()


def test_two_hundred_calls_leave_the_stream_pool_sound(model, monkeypatch):
    """The pool keeps at most 8 idle streams a device; a lookup takes two and a degree one.  A scope that kept a stream
    would leave every later call to make its own; one that gave a stream back twice would hand one stream to both of
    a lookup's roles, or to two handles at once -- the answers below would still have to be right, and are checked."""
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", "1")
    g = pa.parse_bytes(GFA)
    other = pa.parse_bytes(GFA)
    other.to_device(0)  # (a handle that keeps a pool stream of its own meanwhile)
    for i in range(100):
        assert g.gaf_seqs(GOOD) == model["seqs"], i
        assert g.degree().tolist() == model["degree"].tolist(), i
        if i % 25 == 0:  # a refused lookup among them
            with pytest.raises(pa.FlatGFAError):
                g.gaf_seqs(BAD)
            d, _ = other.seg_depth_with_uniq()
            assert np.array_equal(d, fo.seg_depth_with_uniq(model["pools"])[0])
    other.close()
    g.close()
