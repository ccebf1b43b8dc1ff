"""validate and degree at the kernels' own edges (tests/topology_shapes.py: lane, wave, tile and grid-stride-round edges, short
paths, overlapping spans, rows at the linear-probe threshold, empty pools, 70 000 link ends on one segment), against
tests/topology_model.py and the shapes' hand-derived answers.  Run with -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import topology_model as tm
import topology_shapes as ts
from test_gpu_topology import FGFA, load_pools, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sh", ts.SHAPES, ids=lambda s: s.name)
def test_shape(sh):
    p = sh.pools()
    g, flat = load_pools(p)
    try:
        want = same(g, p, sh.name)
        got = g.validate()
        where = list(zip(got["path"].tolist(), got["step"].tolist()))
        if sh.missing is not None:
            assert where == sh.missing
        else:
            assert len(where) == sh.n_missing and where[-1] == sh.last
            assert where == sorted(where) and len(set(where)) == len(where)  # path order, then step order, each pair once
        if sh.name not in ts.BIG:
            r = subprocess.run([FGFA, "-i", flat, "validate"], capture_output=True, timeout=120)
            assert r.returncode == 0 and r.stdout == tm.records_text(p, want), r.stderr
            r = subprocess.run([FGFA, "-i", flat, "degree"], capture_output=True, timeout=120)
            assert r.returncode == 0 and r.stdout == tm.degree_text(p), r.stderr
        if sh.name == "grid_round_paths":  # the same graph, resident: the steps are read in place
            g.to_device()
            assert g.validate().tobytes() == want.tobytes()
    finally:
        g.close()
        os.unlink(flat)


def test_all_pairs_missing_over_more_than_one_round():
    # no links, 2.4 million steps in paths of every length from 0 up: N - P' records (P' the paths that have a step), the last
    # one the last pair of the last path
    n = ts.BIG_N
    cuts = np.unique(np.concatenate([[0, n], np.random.default_rng(7).integers(0, n, 3000), [ts.ROUND, ts.ROUND + 1, ts.TILE]]))
    spans = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])] + [(n, n), (5, 5)]
    p = ts.make_pools(64, ts.fwd(np.arange(n) % 64), spans, [])
    g, flat = load_pools(p)
    try:
        want = tm.validate(p)
        assert len(want) == n - (len(spans) - 2)
        got = g.validate()
        assert got.tobytes() == want.tobytes()
        assert (int(got[-1]["path"]), int(got[-1]["step"])) == (len(spans) - 3, spans[-3][1] - spans[-3][0] - 2)
        assert g.validate_count() == len(want)
        assert np.array_equal(g.degree(), np.zeros(64, np.uint64))
    finally:
        g.close()
        os.unlink(flat)


def test_links_past_one_round_and_scattered_rows():
    # 700 000 links: the link passes go round their grid twice; the degrees and every row against the model
    rng = np.random.default_rng(8)
    S, L = 150_000, 700_001
    links = np.stack([rng.integers(0, 2 * S, L), rng.integers(0, 2 * S, L)], axis=1).astype(np.uint32)
    links[:70_000, 0] = 2 * 77  # a hub row of 70 000 among them
    n = 400_000
    idx = rng.integers(0, L, n // 2)
    steps = np.empty(n, np.uint32)
    steps[0::2], steps[1::2] = links[idx, 0], links[idx, 1]
    flip = rng.random(n // 2) < 0.5  # half of the pairs walk their link backwards
    a, b = steps[0::2].copy(), steps[1::2].copy()
    steps[0::2], steps[1::2] = np.where(flip, b ^ 1, a), np.where(flip, a ^ 1, b)
    p = ts.make_pools(S, steps, [(0, n // 2), (n // 2, n)], [])
    p = ts.with_links(p, links)
    g, flat = load_pools(p)
    try:
        want = same(g, p, "scattered")
        assert 0 < len(want) < n // 2 and (want["step"] % 2 == 1).all()  # the planted pairs are all supported; in between, few are
    finally:
        g.close()
        os.unlink(flat)
