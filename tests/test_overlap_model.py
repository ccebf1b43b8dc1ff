"""The CPU model of path overlap (tests/overlap_model.py) pinned to the C oracle and to slow_odgi's goldens, and the closed-form
answers of tests/overlap_shapes.py pinned to the model.  No GPU."""
import glob
import os
import re

import numpy as np
import pytest

import overlap_model as om
import overlap_shapes as osh
from conftest import GOLDEN
from oracle import flatgfa_oracle as fo


def pools(steps, begin, end, n_segs):
    segs = np.zeros(n_segs, fo.SEG_DT)
    paths = np.zeros(len(begin), fo.PATH_DT)
    paths["steps_start"], paths["steps_end"] = begin, end
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=paths, links=np.zeros(0, fo.LINK_DT), steps=np.asarray(steps, np.uint32),
                    seq_data=z, overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=z,
                    optional_data=z, line_order=z)


def random_graph(seed):
    """Arbitrary spans over one step array: overlapping, nested, empty, repeated steps, few segments."""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, 40))
    N = int(rng.integers(0, 120))
    steps = rng.integers(0, 2 * S, N).astype(np.uint32)
    if N and seed % 3 == 0:
        steps[rng.integers(0, N, N // 3)] = steps[0]  # a handle many times over
    P = int(rng.integers(1, 30))
    if seed % 2 or N == 0:
        a, c = rng.integers(0, N + 1, P), rng.integers(0, N + 1, P)
        b, e = np.minimum(a, c), np.maximum(a, c)
    else:  # back to back, some empty
        cut = np.sort(rng.integers(0, N + 1, P + 1))
        b, e = cut[:-1], cut[1:]
    q = rng.integers(0, P, int(rng.integers(0, 2 * P + 1)))
    return steps, b.astype(np.uint32), e.astype(np.uint32), S, q.astype(np.uint32)


@pytest.mark.parametrize("seed", range(300))
def test_model_matches_oracle_on_random_graphs(seed):
    steps, b, e, S, q = random_graph(seed)
    want = fo.path_touches(pools(steps, b, e, S), q)
    assert np.array_equal(om.touch_rows(steps, b, e, S, q), want)
    assert np.array_equal(om.touch_sparse(steps, b, e, S, q), want)


def test_model_sorted_lookup_matches_marks():
    steps, b, e, S, q = random_graph(4)
    keep = om.MARK_MAX
    try:
        om.MARK_MAX = 0  # (the lookup the limit shapes take)
        assert np.array_equal(om.touch_rows(steps, b, e, S, q), fo.path_touches(pools(steps, b, e, S), q))
    finally:
        om.MARK_MAX = keep


def emit(p, ids, touch):
    """fo.overlap_table's emit (slow_odgi/overlap.py:17-32) over a touch matrix of the caller's."""
    import ctypes
    ids = np.asarray(ids, np.uint32)
    ln, _ = fo.path_depth(p, ids)
    paths, names = fo._c(p.paths), fo._c(p.name_data)
    touch = np.ascontiguousarray(touch, np.uint8)
    n = ctypes.c_uint64(0)
    ptr = fo.lib().oracle_emit_overlap(fo._ptr(paths), fo._ptr(names), len(paths), fo._ptr(ids), len(ids), fo._ptr(ln),
                                       fo._ptr(touch) if touch.size else None, ctypes.byref(n))
    out = ctypes.string_at(ptr, n.value)
    fo.lib().oracle_free(ptr)
    return out


@pytest.mark.parametrize("tsv", sorted(glob.glob(os.path.join(GOLDEN, "*.overlap.tsv"))), ids=lambda x: os.path.basename(x)[:-12])
def test_model_matches_slow_odgi_goldens(tsv):
    with open(tsv[:-12] + ".gfa", "rb") as f:
        p = fo.parse_gfa(f.read())
    with open(tsv, "rb") as f:
        want = f.read()
    P = len(p.paths)
    ids = np.arange(P, dtype=np.uint32)  # (every path, as tests/test_gpu_next_rows.py asks the product)
    b, e, S = p.paths["steps_start"], p.paths["steps_end"], len(p.segs)
    for fn in (om.touch_rows, om.touch_sparse):
        t = fn(p.steps, b, e, S, ids)
        assert np.array_equal(t, fo.path_touches(p, ids))
        assert emit(p, ids, t) == want


def test_constants_are_the_kernels():
    with open(osh.HIP) as f:
        src = f.read()
    assert (osh.WIN_SEGS, osh.BLOCK, osh.COARSE_MAX_WORDS, osh.MAX_SEGS) == (1_179_648, 2048, 8192, 1 << 28)
    launches = re.findall(r"hipLaunchKernelGGL\((k_\w+),.*?n_cus\s*\*\s*(\d+)u", src, re.S)
    assert launches == [("k_coarse_bits", str(osh.COARSE_WG_PER_CU)), ("k_handle_bits", str(osh.BITS_WG_PER_CU)),
                        ("k_pair_touch", str(osh.PAIR_WG_PER_CU))]
    assert "i += 64" in src and "ballot_w64" in src and osh.PAIR_THREADS == 256
    assert re.search(r"dense_max\s*=\s*1ull\s*<<\s*30", src)


def test_host_arithmetic_at_the_limits():
    S = osh.MAX_SEGS
    assert (osh.cwords(S), osh.words(S), osh.per_query(S), osh.n_win(S)) == (8192, 1 << 23, 64 << 20, 228)
    assert osh.batches(S, 24, 24) == [(0, 16), (16, 8)]
    assert osh.batches(8 << 20, 1200, 1200) == [(0, 512), (512, 512), (1024, 176)]
    for S in osh.REFUSED:
        assert osh.cwords(S) > osh.COARSE_MAX_WORDS
    # the wrap the fix removed: words computed in 32 bits is 0 from 2^32 - 31 on
    old = lambda S: ((((S + 31) & 0xFFFFFFFF) // 32) + 3) & ~3 & 0xFFFFFFFF  # noqa: E731
    assert [old(S) == 0 for S in osh.REFUSED] == [False, False, False, True, True]


def reaches(s: osh.Shape, n_cus: int):
    """What each shape is there for, at this CU count: {threshold: reached}."""
    S, P, n_q = s.n_segs, s.P, len(s.queries)
    bs = osh.batches(S, P, n_q, s.dense_max)
    dense = osh.all_paths(S, P, s.dense_max)
    jobs = max((P if dense else nq) * 2 * osh.n_win(S) for _, nq in bs)
    pairs = max(nq * P for _, nq in bs)
    return {"coarse_stride": P > osh.COARSE_WG_PER_CU * n_cus, "bits_stride": jobs > osh.BITS_WG_PER_CU * n_cus,
            "pair_stride": pairs > osh.PAIR_WG_PER_CU * n_cus * osh.PAIR_THREADS // 64, "ballot_round_2": osh.cwords(S) > osh.BALLOT,
            "windows_3": osh.n_win(S) >= 3, "batches_3": len(bs) >= 3, "dense": dense}


@pytest.mark.parametrize("n_cus", [8, 256])
def test_shapes_reach_their_thresholds(n_cus):
    r = {name: reaches(f(), n_cus) for name, f in osh.catalog(n_cus)}
    for k in ("coarse_stride", "bits_stride", "pair_stride", "ballot_round_2", "windows_3", "batches_3"):
        assert r["grid_batches"][k], k
    assert not r["grid_batches"]["dense"]
    assert r["grid_dense"]["dense"] and r["grid_dense"]["bits_stride"] and r["grid_dense"]["coarse_stride"]
    assert r["edges"]["ballot_round_2"] and r["edges"]["windows_3"] and r["edges"]["dense"]
    assert r["batch_edges"]["batches_3"] and not r["batch_edges"]["dense"]
    assert r["limit"]["windows_3"] and not r["limit"]["dense"] and r["limit_dense"]["dense"]


@pytest.mark.parametrize("n_cus", [8, 256])
@pytest.mark.parametrize("name", [n for n, _ in osh.catalog()])
def test_shape_closed_form_matches_model(name, n_cus):
    s = dict(osh.catalog(n_cus))[name]()
    assert len(s.steps) < 1 << 32 and int(s.steps.max()) >> 1 < s.n_segs
    assert (s.begin <= s.end).all() and (s.end <= len(s.steps)).all()
    got = om.touch_sparse(s.steps, s.begin, s.end, s.n_segs, s.queries)
    rows = np.unique(np.concatenate([np.arange(min(40, len(s.queries))), [len(s.queries) - 1]]))
    assert np.array_equal(om.touch_rows(s.steps, s.begin, s.end, s.n_segs, s.queries[rows]), got[rows])
    if s.want is not None:
        assert np.array_equal(got, s.want)
        assert 0 < int(s.want.sum()) < s.want.size
    else:
        assert 0 < int(got.sum()) < got.size


def test_planted_layout():
    s = osh.step_layout()
    b, e = s.begin.astype(np.int64), s.end.astype(np.int64)
    n = e - b
    for L in range(8):  # every length 0..7 at every begin offset mod 4
        assert set((b[n == L] % 4).tolist()) == {0, 1, 2, 3}, L
    bait = int(s.steps[0])
    laid = np.argsort(b, kind="stable")
    for p in laid[:-8]:  # (the spans given by hand lie in one block at the end)
        if n[p]:
            assert (s.steps[b[p] - 4:b[p]] == bait).all() and (s.steps[e[p]:e[p] + 4] == bait).all()
    assert (n == 0).sum() >= 3
    assert s.want[:, 0].sum() == 0  # the bait path touches nobody
