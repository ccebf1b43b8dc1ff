"""validate and degree on the GPU (flatgfa_validate, flatgfa_degree and their tables, `fgfa validate`, `fgfa degree`,
FlatGFA.validate / degree) against tests/topology_model.py, byte for byte: the golden graphs as they stand and with 90 % of
their links dropped, the synthetic graph against the reference's pinned output, and the project's own chop and extract
outputs.  Run with -m gpu."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import chop_model as cm
import pollen_amd as pa
import topology_model as tm
import topology_shapes as ts
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
TOPO = os.path.join(GOLDEN, "topology")


def parsable():
    out = []
    for path in golden_gfas():
        try:
            pa.parse(path).close()
        except Exception:
            continue
        out.append(path)
    return out


def load_pools(p: fo.Pools):
    fd, path = tempfile.mkstemp(suffix=".flatgfa")
    with os.fdopen(fd, "wb") as f:
        f.write(fo.dump_flatgfa(p))
    return pa.load(path), path


def same(g, p: fo.Pools, what):
    """Records, count, both tables and the degrees of handle g against the model on pools p."""
    want = tm.validate(p)
    got = g.validate()
    assert got.dtype.names == ("path", "step", "src", "dst")
    assert got.tobytes() == want.tobytes(), what
    assert g.validate_count() == len(want), what
    assert g.validate_table() == tm.records_text(p, want), what
    d = g.degree()
    assert d.dtype == np.uint64 and np.array_equal(d, tm.degree(p)), what
    assert g.degree_table() == tm.degree_text(p), what
    return want


def cli(args, **kw):
    return subprocess.run([FGFA] + args, capture_output=True, timeout=120, **kw)


@pytest.mark.parametrize("path", parsable(), ids=fixture_id)
def test_golden_original_and_dropped(path):
    name = fixture_id(path)
    for gfa in (path, os.path.join(TOPO, name + ".dropped.gfa")):
        g = pa.parse(gfa)
        p = cm.pools_of(g)
        same(g, p, gfa)
        # the library parses what the reference parsed (every line is terminated): its text is the reference's own
        if open(gfa, "rb").read().endswith(b"\n"):
            ref = os.path.join(TOPO, name + (".dropped.validate.txt" if gfa != path else ".validate.txt"))
            assert g.validate_table() == open(ref, "rb").read()
            if gfa == path:
                assert g.degree_table() == open(os.path.join(TOPO, name + ".degree.tsv"), "rb").read()
        r = cli(["-I", gfa, "validate"])
        assert r.returncode == 0 and r.stdout == tm.validate_text(p), r.stderr
        r = cli(["-I", gfa, "degree"])
        assert r.returncode == 0 and r.stdout == tm.degree_text(p), r.stderr
        with tempfile.TemporaryDirectory() as d:
            flat = os.path.join(d, "g.flatgfa")
            g.write_flatgfa(flat)
            r = cli(["-i", flat, "validate"])
            assert r.returncode == 0 and r.stdout == tm.validate_text(p), r.stderr
            r = cli(["-i", flat, "degree"])
            assert r.returncode == 0 and r.stdout == tm.degree_text(p), r.stderr
        g.close()


def test_done_when_lines():
    r = cli(["-I", os.path.join(GOLDEN, "ref_ex2.gfa"), "validate"])
    assert r.returncode == 0 and r.stdout == b""
    r = cli(["-I", os.path.join(TOPO, "ref_ex2.dropped.gfa"), "validate"])
    want = open(os.path.join(TOPO, "ref_ex2.dropped.validate.txt"), "rb").read()
    assert r.returncode == 0 and r.stdout == want and want.count(b"\n") == 8
    r = cli(["-I", os.path.join(GOLDEN, "ref_ex2.gfa"), "degree"])
    assert r.returncode == 0 and r.stdout == open(os.path.join(TOPO, "ref_ex2.degree.tsv"), "rb").read()


def test_synthetic_graph_against_the_reference():
    import json
    manifest = json.load(open(os.path.join(TOPO, "MANIFEST.json")))
    p = ts.synth_mid()
    g, flat = load_pools(p)
    try:
        same(g, p, "synth_mid")
        assert hashlib.sha256(g.validate_table()).hexdigest() == manifest["synth_mid.validate.txt"]["sha256"]
        assert hashlib.sha256(g.degree_table()).hexdigest() == manifest["synth_mid.degree.tsv"]["sha256"]
        r = cli(["-i", flat, "validate"])
        assert r.returncode == 0 and hashlib.sha256(r.stdout).hexdigest() == manifest["synth_mid.validate.txt"]["sha256"]
        # from GFA text on stdin
        r = cli(["degree"], input=ts.gfa_text(p))
        assert r.returncode == 0 and hashlib.sha256(r.stdout).hexdigest() == manifest["synth_mid.degree.tsv"]["sha256"]
    finally:
        g.close()
        os.unlink(flat)


@pytest.mark.parametrize("path", parsable(), ids=fixture_id)
def test_chop_and_extract_outputs_validate_as_the_model_says(path):
    g = pa.parse(path)
    try:
        c = g.chop(3, links=True)
    except pa.FlatGFAError:
        c = None  # (a fixture chop refuses)
    if c is not None:
        same(c, cm.pools_of(c), "chop")
        same(g.chop(3, links=False), cm.pools_of(g.chop(3, links=False)), "chop without links")
    p = cm.pools_of(g)
    for name in sorted({int(s["name"]) for s in p.segs})[:4]:
        for dist in (0, 1, 3):
            q = g.extract(name, dist)
            same(q, cm.pools_of(q), ("extract", name, dist))
    g.close()


def test_chop_of_a_valid_graph_stays_valid():
    p = ts.synth_mid()
    full = ts.with_links(p, ts.induced_links(p, ts.SYNTH_MID["form_salt"], 0, 0))
    g, flat = load_pools(full)
    try:
        assert g.validate_count() == 0 and g.validate_table() == b""
        c = g.chop(3, links=True)
        cp = cm.pools_of(c)
        assert len(cp.segs) > len(full.segs)
        assert len(same(c, cp, "chopped")) == 0
        assert c.chop(3, links=False).validate_count() == len(cp.steps) - len(cp.paths)
    finally:
        g.close()
        os.unlink(flat)


def test_resident_and_host_handles_agree_and_depth_is_undisturbed():
    p = ts.synth_mid()
    g, flat = load_pools(p)
    try:
        want = same(g, p, "host")
        g.to_device()
        d0, u0 = g.seg_depth_with_uniq()
        wd, wu = fo.seg_depth_with_uniq(p)
        assert np.array_equal(d0, wd) and np.array_equal(u0, wu)
        assert same(g, p, "resident").tobytes() == want.tobytes()
        d1, u1 = g.seg_depth_with_uniq()
        assert np.array_equal(d1, wd) and np.array_equal(u1, wu)
        ln, mean = g.path_depth()
        wl, wm = fo.path_depth(p)
        assert np.array_equal(ln, wl) and mean.tobytes() == wm.tobytes()
    finally:
        g.close()
        os.unlink(flat)
    # resident before the index exists: the first validate builds it beside the plan
    h, flat = load_pools(p)
    try:
        h.to_device()
        same(h, p, "resident first")
        d, u = h.seg_depth_with_uniq()
        assert np.array_equal(d, wd) and np.array_equal(u, wu)
    finally:
        h.close()
        os.unlink(flat)


def _validate_rc(g, out=True):
    o, n = ctypes.c_void_p(), ctypes.c_uint64(123)
    rc = _lib.lib().flatgfa_validate(g._h, ctypes.byref(o) if out else None, ctypes.byref(n))
    if o.value:
        _lib.lib().flatgfa_missing_links_free(o)
    return rc, n.value


def test_refusals_leave_the_handle_usable():
    lib = _lib.lib()
    text = b"S\t1\tACGT\nS\t2\tAC\nP\tp\t1+,2+,1-\t*\nL\t1\t+\t2\t+\t0M\n"
    g = pa.parse_bytes(text)
    p = cm.pools_of(g)
    # a link naming a segment that is not there (the handle's own link pool, overwritten in place): refused, and no index is kept
    data, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.flatgfa_pool(g._h, 3, ctypes.byref(data), ctypes.byref(n), None) == 0 and n.value == 1
    good = ctypes.c_uint32.from_address(data.value + 4).value
    ctypes.c_uint32.from_address(data.value + 4).value = 9 << 1
    assert _validate_rc(g) == (-2, 0)
    with pytest.raises(pa.FlatGFAError, match="link") as e:
        g.degree()
    assert e.value.code == -2
    ctypes.c_uint32.from_address(data.value + 4).value = good
    want = same(g, p, "after a bad link")
    assert [(int(r["step"]), int(r["src"]), int(r["dst"])) for r in want] == [(1, 2, 1)]
    g.close()
    # a step naming a segment that is not there
    bad = fo.Pools(**{k: getattr(p, k).copy() for k in fo.POOL_ORDER})
    bad.steps[2] = 7 << 1
    h, path = load_pools(bad)
    try:
        for _ in range(2):
            with pytest.raises(pa.FlatGFAError, match="step") as e:
                h.validate()
            assert e.value.code == -2
            assert _validate_rc(h, out=False) == (-2, 0)
        assert np.array_equal(h.degree(), tm.degree(bad))  # the links are sound: the handle still answers
        with pytest.raises(pa.FlatGFAError):
            h.validate_table()
    finally:
        h.close()
        os.unlink(path)
    # a lone bad step in a path of one step is found too
    bad1 = ts.make_pools(2, [9 << 1, 0, 2], [(0, 1), (1, 3)], [(0, 2)])
    h, path = load_pools(bad1)
    try:
        assert _validate_rc(h)[0] == -2
    finally:
        h.close()
        os.unlink(path)
    # a path whose span leaves the pool
    span = fo.Pools(**{k: getattr(p, k).copy() for k in fo.POOL_ORDER})
    g2 = pa.parse_bytes(text)
    pd, pn = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.flatgfa_pool(g2._h, 2, ctypes.byref(pd), ctypes.byref(pn), None) == 0 and pn.value == 1
    ctypes.c_uint32.from_address(pd.value + 12).value = 4  # steps_end of 3 steps
    assert _validate_rc(g2)[0] == -2
    ctypes.c_uint32.from_address(pd.value + 12).value = 3
    same(g2, span, "after a bad span")
    # NULL arguments
    o, c = ctypes.c_void_p(), ctypes.c_uint64()
    sz = ctypes.c_size_t()
    assert lib.flatgfa_validate(None, ctypes.byref(o), ctypes.byref(c)) == -1
    assert lib.flatgfa_validate(g2._h, ctypes.byref(o), None) == -1
    assert lib.flatgfa_validate_table(g2._h, None, ctypes.byref(sz)) == -1
    assert lib.flatgfa_validate_table(None, ctypes.byref(o), ctypes.byref(sz)) == -1
    assert lib.flatgfa_degree(g2._h, None) == -1 and lib.flatgfa_degree(None, None) == -1
    assert lib.flatgfa_degree_table(g2._h, None, None) == -1
    lib.flatgfa_missing_links_free(None)
    assert lib.flatgfa_validate(g2._h, None, ctypes.byref(c)) == 0 and c.value == 1  # the count alone
    g2.close()


@pytest.mark.parametrize("args", [["validate", "x"], ["degree", "-d"]])
def test_cli_usage_errors(args):
    r = cli(args, input=b"S\t1\tA\n")
    assert r.returncode == 2 and r.stdout == b"" and b"usage" in r.stderr


def test_cli_exit_status_is_zero_when_links_are_missing():
    r = cli(["validate"], input=b"S\t1\tA\nS\t2\tC\nP\tx\t1+,2-\t*\n")
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == b"[odgi::validate] error: the path x does not respect the graph topology: the link 1+,2- is missing.\n"
