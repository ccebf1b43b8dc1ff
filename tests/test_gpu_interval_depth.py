"""Interval and window depth over many paths on the GPU (flatgfa_intervals_depth, flatgfa_window_depth_paths_table,
flatgfa_bed_depth_paths_table; `fgfa window-depth-all`, `fgfa depth --bed-paths`).

The vectors are compared with the model (tests/interval_model.py: the oracle's interval_depth, group by group) by
.tobytes(): no tolerance.  Every shape of tests/interval_shapes.py goes through the Python method with the lane / wave cut as
it ships, with every interval on the wave kernel and with every interval on one lane; the stand-alone program
(tests/device_check/interval_check.hip, built with the library) runs the job with the batch budget lowered, and on raw arrays
whose products and widths no f64 holds (big_products: the closed form in Python integers is the reference).  Run with -m gpu."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import interval_model as im
import interval_shapes as ish
import pollen_amd as pa
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
EXE = os.path.join(ROOT, "pollen_amd", "build", "interval_check")
CUT_HOOK = "FLATGFA_INTERVAL_LANE_CUT"
SHAPES = [f.__name__ for f in ish.SHAPES]


def read(path):
    with open(path, "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def want(name: str):
    """{label: the model's bytes} of a shape, computed once."""
    s = ish.shape(name)
    return {label: im.intervals_depth(s.pools, ids, st, en).tobytes() for label, (ids, st, en) in s.lists.items()}


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("interval_shapes")
    out = {}
    for name in SHAPES:
        out[name] = str(d / (name + ".flatgfa"))
        with open(out[name], "wb") as f:
            f.write(fo.dump_flatgfa(ish.shape(name).pools))
    return out


def check_shape(images, name):
    s = ish.shape(name)
    g = pa.load(images[name])
    try:
        for label, (ids, st, en) in s.lists.items():
            got = g.intervals_depth(ids, st, en)
            w = np.frombuffer(want(name)[label], np.float64)
            assert got.tobytes() == w.tobytes(), (name, label, np.flatnonzero(got != w)[:5], got[got != w][:5], w[got != w][:5])
    finally:
        g.close()


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(images, name, monkeypatch):
    monkeypatch.delenv(CUT_HOOK, raising=False)
    check_shape(images, name)


@pytest.mark.parametrize("cut", [0, 1 << 30], ids=["all_waves", "all_lanes"])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_on_one_class(images, name, cut, monkeypatch):
    monkeypatch.setenv(CUT_HOOK, str(cut))
    check_shape(images, name)


# ---- the job on its own: batch budget, cut ----

def case_bytes(pools, ids, st, en, budget, cut, depth=None) -> bytes:
    depth = fo.seg_depth(pools) if depth is None else depth
    ids = np.ascontiguousarray(ids, np.uint32)
    pad = np.zeros(len(ids) & 1, np.uint32)
    head = struct.pack("<6Q", len(pools.segs), len(pools.steps), len(pools.paths), len(ids), budget, cut)
    parts = [pools.seg_lens().astype(np.uint32), np.asarray(depth).astype(np.uint32), pools.steps.astype(np.uint32),
             pools.paths["steps_start"].astype(np.uint32), pools.paths["steps_end"].astype(np.uint32), ids, pad,
             np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(en, np.uint64)]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def job_cases():
    """(id, input bytes, n, the model's bytes or None for an error, return code, batches or None)"""
    b = ish.shape("basic")
    out = []
    for k, (label, groups, budget, batches) in enumerate(ish.budget_cases()):
        ids, st, en = ish.budget_list(label, groups, 40 + k)
        for cut in (ish.LANE_CUT, 0):
            out.append(("%s-cut%d" % (label, cut), case_bytes(b.pools, ids, st, en, budget, cut), len(ids),
                        im.intervals_depth(b.pools, ids, st, en).tobytes(), 0, batches))
    t = ish.shape("tiles")
    ids, st, en = t.lists["all_paths"]
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in t.pools.paths]
    groups = [int(ids[a]) for a, _ in im.runs(ids)]
    for budget in (2 * ish.TILE + 1, 3 * ish.TILE):  # every path alone; two or three paths a batch, the scan restarting inside tiles
        out.append(("tiles-%d" % budget, case_bytes(t.pools, ids, st, en, budget, ish.LANE_CUT), len(ids), want("tiles")["all_paths"], 0,
                    ish.plan_batches(groups, lengths, budget)))
    # three thousand slots: a batch cut at both ends of a run of stepless paths, batches of a tile that end in such a run
    m = ish.shape("many_paths")
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in m.pools.paths]
    for label, name, budget, _ in ish.run_budget_cases():
        ids, st, en = m.lists[name]
        groups = [int(ids[a]) for a, _ in im.runs(ids)]
        out.append(("many_paths-" + label, case_bytes(m.pools, ids, st, en, budget, ish.LANE_CUT), len(ids), want("many_paths")[name], 0,
                    ish.plan_batches(groups, lengths, budget)))
    # one long group, and groups with heads on the tile seams, a batch per new path: M comes from one scan over all batches
    lg = ish.shape("long_groups")
    lengths = [int(p["steps_end"]) - int(p["steps_start"]) for p in lg.pools.paths]
    for name in ("tile_seams", "heads"):
        ids, st, en = lg.lists[name]
        groups = [int(ids[a]) for a, _ in im.runs(ids)]
        out.append(("long_groups-%s-budget1" % name, case_bytes(lg.pools, ids, st, en, 1, ish.LANE_CUT), len(ids), want("long_groups")[name], 0,
                    ish.plan_batches(groups, lengths, 1)))
    # lengths and depths up to 2^32 - 1, widths up to 2^64 - 1: where u64 -> f64 rounds.  Raw arrays (no handle loads such
    # segments); the closed form in Python integers is the reference
    pools, depth, ids, st, en = ish.big_products()
    model = im.closed_form(pools, ids, st, en, depth).tobytes()
    for cut in (ish.LANE_CUT, 0):
        out.append(("big_products-cut%d" % cut, case_bytes(pools, ids, st, en, 1 << 27, cut, depth), len(ids), model, 0, 1))
    # a step that names no segment: FLATGFA_ERR_BOUNDS, whatever the intervals
    bad = fo.Pools(**{n: getattr(b.pools, n) for n in fo.POOL_ORDER})
    bad.steps = b.pools.steps.copy()
    bad.steps[100] = (len(b.pools.segs) << 1) | 1
    ids, st, en = b.lists["p0_whole"]
    out.append(("bad_step", case_bytes(bad, ids, st, en, 1 << 27, ish.LANE_CUT, fo.seg_depth(b.pools)),
                len(ids), None, -2, None))
    out.append(("bad_path_id", case_bytes(b.pools, [0, 4, 0], [0, 0, 0], [5, 5, 5], 1 << 27, ish.LANE_CUT), 3, None, -2, None))
    out.append(("no_intervals", case_bytes(b.pools, [], [], [], 1 << 27, ish.LANE_CUT), 0, b"", 0, 0))
    return out


@pytest.fixture(scope="module")
def job_outputs(tmp_path_factory):
    subprocess.run(["make", "-C", CSRC, "interval_check"], check=True, capture_output=True, timeout=600)
    d = tmp_path_factory.mktemp("interval_check")
    cases = job_cases()
    lines = []
    for k, c in enumerate(cases):
        (d / ("%d.in" % k)).write_bytes(c[1])
        lines.append("%s %s\n" % (d / ("%d.in" % k), d / ("%d.out" % k)))
    (d / "manifest.txt").write_text("".join(lines))
    r = subprocess.run([EXE, str(d / "manifest.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == "interval_check: %d cases" % len(cases)
    return {c[0]: (c, (d / ("%d.out" % k)).read_bytes()) for k, c in enumerate(cases)}


JOB_IDS = ["%s-cut%d" % (c[0], cut) for c in ish.budget_cases() for cut in (ish.LANE_CUT, 0)] + \
    ["tiles-%d" % (2 * ish.TILE + 1), "tiles-%d" % (3 * ish.TILE)] + \
    ["many_paths-runs-budget1", "many_paths-budget1024", "many_paths-budget2048", "long_groups-tile_seams-budget1", "long_groups-heads-budget1",
     "big_products-cut%d" % ish.LANE_CUT, "big_products-cut0", "bad_step", "bad_path_id", "no_intervals"]


@pytest.mark.parametrize("case", JOB_IDS)
def test_job_with_lowered_budget(job_outputs, case):
    (_, _, n, model, rc, batches), got = job_outputs[case]
    got_rc, got_batches = struct.unpack("<qQ", got[:16])
    assert got_rc == rc, case
    assert got[16 + 8 * n:] == b"\xa5" * (8 * 64), "a store past the results"
    if model is not None:
        assert got[16:16 + 8 * n] == model, (case, np.frombuffer(got[16:16 + 8 * n], np.float64), np.frombuffer(model, np.float64))
        assert got_batches == batches, case


def test_job_cases_are_the_listed_ones():
    assert [c[0] for c in job_cases()] == JOB_IDS


# ---- golden graphs: the tables ----

def parsable_gfas():
    out = []
    for gfa in golden_gfas():
        try:
            fo.parse_gfa(read(gfa))
            out.append(gfa)
        except fo.ParseError:
            pass
    return out


def shuffled_bed(pools, seed) -> bytes:
    """Every path named, in shuffled blocks of one to four entries; a comment line; names that come back later."""
    rng = np.random.default_rng(seed)
    lens, _ = fo.path_depth(pools)
    order = list(rng.permutation(len(pools.paths))) * 2
    rng.shuffle(order)
    lines = [b"#path\tstart\tend"]
    for p in order:
        for _ in range(int(rng.integers(1, 5))):
            a = int(rng.integers(0, int(lens[p]) + 2))
            lines.append(b"%s\t%d\t%d" % (pools.path_name(int(p)), a, a + int(rng.integers(0, int(lens[p]) + 3))))
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("gfa", parsable_gfas(), ids=fixture_id)
def test_golden_tables(gfa, tmp_path, monkeypatch):
    monkeypatch.delenv(CUT_HOOK, raising=False)
    pools = fo.parse_gfa(read(gfa))
    P = len(pools.paths)
    names = [pools.path_name(i) for i in range(P)]
    lens, _ = fo.path_depth(pools)
    g = pa.parse(gfa)
    try:
        for w in sorted({1, 4, max([int(x) for x in lens] + [1])}):
            got = g.window_depth_paths_table(w)
            assert got == b"".join(g.window_depth_table(i, w) for i in range(P)), (w, "the existing route, path by path")
            if len(set(names)) == P:  # (the oracle's table finds a path by its name)
                assert got == im.window_depth_paths_table(pools, w), (w, "the oracle")
            sub = list(range(P - 1, -1, -2))
            assert g.window_depth_paths_table(w, sub) == b"".join(g.window_depth_table(i, w) for i in sub)
        if P:
            bed = shuffled_bed(pools, 7)
            got = g.bed_depth_paths_table(bed)
            assert got == im.bed_depth_paths_table(pools, bed)
            # the CLI prints exactly the C tables
            (tmp_path / "x.bed").write_bytes(bed)
            out = subprocess.run([FGFA, "-I", gfa, "depth", "--bed-paths", str(tmp_path / "x.bed")], capture_output=True, timeout=120)
            assert out.returncode == 0 and out.stdout == got, out.stderr
        out = subprocess.run([FGFA, "-I", gfa, "window-depth-all", "4"], capture_output=True, timeout=120)
        assert out.returncode == 0 and out.stdout == g.window_depth_paths_table(4), out.stderr
    finally:
        g.close()


REPEATED = [[0, 0], [0, 2, 0], [1, 1, 3], [3, 3, 3]]


@pytest.mark.parametrize("graph", ["basic", "edge_names_loops.gfa"])
def test_a_path_listed_again_gets_its_own_table(images, graph, monkeypatch):
    """The window table is the per-path tables one behind another, whatever the list: a path listed twice in a row, or with
    only paths of no windows in between (path 2 of `basic` has no steps), is not one group of both copies' windows."""
    monkeypatch.delenv(CUT_HOOK, raising=False)
    if graph == "basic":
        pools = ish.shape("basic").pools
        g = pa.load(images["basic"])
    else:
        pools = fo.parse_gfa(read(os.path.join(GOLDEN, graph)))
        g = pa.parse(os.path.join(GOLDEN, graph))
    try:
        P = len(pools.paths)
        assert P >= 4 and len({pools.path_name(i) for i in range(P)}) == P
        lens, _ = fo.path_depth(pools)
        for w in (1, 50, int(max(lens)) + 1):
            one = [g.window_depth_table(i, w) for i in range(P)]
            for ids in REPEATED + [[p for p in range(P) for _ in (0, 1)]]:
                got = g.window_depth_paths_table(w, ids)
                assert got == b"".join(one[i] for i in ids), (graph, w, ids, "the one-path route, path by path")
                assert got == im.window_depth_paths_table(pools, w, ids), (graph, w, ids, "the oracle")
            assert g.window_depth_paths_table(w) == b"".join(one), (graph, w, "all paths: no seam")
        if graph == "basic":
            ids, st, en = ish.shape("basic").lists["aba"]
            assert g.intervals_depth(ids, st, en).tobytes() == want("basic")["aba"]
        else:
            st, en = np.zeros(P, np.uint64), lens.astype(np.uint64)
            assert g.intervals_depth(list(range(P)), st, en).tobytes() == im.intervals_depth(pools, list(range(P)), st, en).tobytes()
    finally:
        g.close()


def test_existing_cli_is_unchanged():
    """`fgfa window-depth` prints what it printed: the reference's README vector (`window-depth 5 4`, the path named 5 of
    standin_note5.gfa), the hand-computed tables of kat_window_depth.gfa (its paths are x and y), and, for `5 4` on that
    graph, no table and "path not found"."""
    from test_next_rows_oracle import WINDOW_KATS
    note5 = os.path.join(GOLDEN, "standin_note5.gfa")
    out = subprocess.run([FGFA, "-I", note5, "window-depth", "5", "4"], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout == b"5\t0\t4\t2\n5\t4\t8\t2\n5\t8\t12\t2\n5\t12\t13\t2\n"
    assert out.stdout == fo.window_depth_table(fo.parse_gfa(read(note5)), b"5", 4)
    gfa = os.path.join(GOLDEN, "kat_window_depth.gfa")
    out = subprocess.run([FGFA, "-I", gfa, "window-depth", "5", "4"], capture_output=True, timeout=120)
    assert (out.returncode, out.stdout, out.stderr) == (1, b"", b"fgfa: path not found\n")
    n = 0
    for kind, a, b, table in WINDOW_KATS:
        if kind == "window":
            out = subprocess.run([FGFA, "-I", gfa, "window-depth", a.decode(), str(b)], capture_output=True, timeout=120)
            assert out.returncode == 0 and out.stdout == table, (a, b)
            n += 1
    assert n == 3


def test_order_of_calls(images):
    """The feature writes d_depth: seg_depth and path_depth before, between and after give what they gave."""
    s = ish.shape("basic")
    ids, st, en = s.lists["mixed_groups"]
    w = want("basic")["mixed_groups"]
    d, u = fo.seg_depth_with_uniq(s.pools)
    ln, mean = fo.path_depth(s.pools)
    for first in ("intervals", "seg_depth", "path_depth", "window_table", "subset"):
        g = pa.load(images["basic"])
        try:
            for step in (first, "seg_depth", "intervals", "path_depth", "window_table", "intervals", "subset", "intervals", "seg_depth"):
                if step == "intervals":
                    assert g.intervals_depth(ids, st, en).tobytes() == w, (first, step)
                elif step == "seg_depth":
                    gd, gu = g.seg_depth_with_uniq()
                    assert (gd == d).all() and (gu == u).all() and (g.seg_depth() == d).all(), (first, step)
                elif step == "path_depth":
                    gl, gm = g.path_depth()
                    assert (gl == ln).all() and gm.tobytes() == mean.tobytes(), (first, step)
                elif step == "window_table":
                    assert g.window_depth_paths_table(50) == im.window_depth_paths_table(s.pools, 50), (first, step)
                else:  # (a subset query leaves another vector in d_depth)
                    sd, _ = g.seg_depth_subset([1])
                    assert (sd == fo.seg_depth_subset(s.pools, [1])[0]).all(), (first, step)
        finally:
            g.close()


def test_errors(images):
    g = pa.load(images["basic"])
    lib = _lib.lib()
    try:
        one = np.array([7], np.uint64)
        ids = np.array([0], np.uint32)
        out = np.full(3, -1.0)
        # NULL where data is needed
        assert lib.flatgfa_intervals_depth(None, ids.ctypes.data, one.ctypes.data, one.ctypes.data, 1, out.ctypes.data) == -1
        for args in ((None, one.ctypes.data, one.ctypes.data), (ids.ctypes.data, None, one.ctypes.data), (ids.ctypes.data, one.ctypes.data, None)):
            assert lib.flatgfa_intervals_depth(g._h, *args, 1, out.ctypes.data) == -1
        assert lib.flatgfa_intervals_depth(g._h, ids.ctypes.data, one.ctypes.data, one.ctypes.data, 1, None) == -1
        assert lib.flatgfa_window_depth_paths_table(g._h, None, 0, 4, None, None) == -1
        assert lib.flatgfa_bed_depth_paths_table(g._h, b"p0\t0\t1\n", 7, None, None) == -1
        # n_intervals == 0: OK, with or without arrays
        assert lib.flatgfa_intervals_depth(g._h, None, None, None, 0, None) == 0
        assert len(g.intervals_depth([], [], [])) == 0
        # window == 0
        with pytest.raises(pa.FlatGFAError) as e:
            g.window_depth_paths_table(0)
        assert e.value.code == -1
        # a path id >= path_count: nothing written
        bad = np.array([0, 4, 1], np.uint32)
        three = np.array([0, 0, 0], np.uint64)
        assert lib.flatgfa_intervals_depth(g._h, bad.ctypes.data, three.ctypes.data, (three + 9).ctypes.data, 3, out.ctypes.data) == -2
        assert (out == -1.0).all()
        with pytest.raises(pa.FlatGFAError) as e:
            g.window_depth_paths_table(4, [0, 4])
        assert e.value.code == -2
        # a BED name that is not in the graph: the entry's index
        with pytest.raises(pa.FlatGFAError) as e:
            g.bed_depth_paths_table(b"#c\np0\t0\t4\np1\t0\t4\nnope\t0\t4\np0\t1\t2\n")
        assert e.value.code == -2 and "entry 2 " in _lib.last_error()
        # an empty BED, as flatgfa_bed_depth_table
        for empty in (b"", b"#only a comment\n", b"p0\t0\t4"):
            with pytest.raises(pa.FlatGFAError) as e:
                g.bed_depth_paths_table(empty)
            assert e.value.code == -2 and _lib.last_error() == "BED: no intervals"
        with pytest.raises(pa.FlatGFAError):
            g.intervals_depth([b"nope"], [0], [1])
        with pytest.raises(pa.FlatGFAError):
            g.intervals_depth([0, 1], [0], [1])
        # the handle still answers
        ids, st, en = ish.shape("basic").lists["aba"]
        assert g.intervals_depth(ids, st, en).tobytes() == want("basic")["aba"]
        assert g.intervals_depth([b"p0", b"p1", b"p0"], st, en).tobytes() == want("basic")["aba"]
    finally:
        g.close()


def test_a_step_that_names_no_segment(tmp_path):
    s = ish.shape("basic")
    bad = fo.Pools(**{n: getattr(s.pools, n) for n in fo.POOL_ORDER})
    bad.steps = s.pools.steps.copy()
    bad.steps[100] = (len(s.pools.segs) << 1) | 1
    f = str(tmp_path / "bad.flatgfa")
    with open(f, "wb") as out:
        out.write(fo.dump_flatgfa(bad))
    g = pa.load(f)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            g.intervals_depth([3], [0], [9])  # (whichever path is asked: the node depth reads every step)
        assert e.value.code == -2
    finally:
        g.close()
