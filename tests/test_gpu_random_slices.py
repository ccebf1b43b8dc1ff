"""Random differential slices of crush, flip, flatten, print and validate/degree: the seeded adversarial pools of
tests/random_pools.py -- several of the kernels' edges in one case, where the geometry files plant one at a time -- through
the helpers the features' own GPU tests use, byte for byte against the models.  One test per feature and seed; each runs all
of its seed's cases, skips none, and ends on the number of cases it ran and on the census of the classes they reached
(tests/test_random_pools.py holds the same census on the CPU).  A failure names random_pools.make's arguments.  Run with -m gpu."""
import os

import numpy as np
import pytest

import crush_gpu as cg
import crush_model as cm
import flatten_model as flm
import flip_gpu as fg
import flip_model as fm
import parse_shapes
import pollen_amd as pa
import print_model as pm
import random_pools as rp
import topology_model as tm
from pollen_amd import device as pdev
from test_gpu_flatten_geometry import load
from test_gpu_flip_geometry import round_sizes
from test_gpu_topology import load_pools, same

pytestmark = pytest.mark.gpu
FLATTEN_HOOK, PRINT_HOOK = "FLATGFA_FLATTEN_CHUNK_LINES", "FLATGFA_PRINT_CHUNK_ITEMS"  # (both are read at every call)


def run(feature, seed, one):
    """one(k, pools, extras, what) for every case of the seed; then the count and the census."""
    total = {c: 0 for c in rp.CLASSES[feature]}
    ran = 0
    for k in range(rp.CASES[feature]):
        sd = rp.case_seed(seed, k)
        p, ex = rp.make(sd, feature), rp.extras(sd, feature)
        one(k, p, ex, "%s, seed %d, case %d: random_pools.make(%d, %r)" % (feature, seed, k, sd, feature))
        for c, v in rp.census(p, feature, **ex).items():
            total[c] += v
        ran += 1
    print("%s, seed %d: %d cases; %s" % (feature, seed, ran, "; ".join("%s: %d" % cv for cv in total.items())))
    assert ran == rp.CASES[feature]
    assert all(total.values()), total


def hook(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_crush(seed, tmp_path):
    def one(k, p, ex, what):
        want = cm.crush_fast(p)
        cg.check_device_pair(p, want, what=what)
        with load(p, tmp_path) as g, g.crush() as q:
            cm.assert_same_pools(cm.pools_of(q), want, what)
    run("crush", seed, one)


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_flip(seed):
    def one(k, p, ex, what):
        want = fm.flip(p)
        fg.check_device_pair(p, want, what=what)
        fg.check_handle(p, want, what=what)
        sizes, _ = round_sizes(p)
        if k % 2 and sizes:  # the key table in more than one round
            r = sizes[(k // 2) % len(sizes)]
            dg, links, align = fg.to_device(p)
            new, links_out, _ = pdev.flip(dg, links, alignment=align, round_keys=r)
            assert np.array_equal(fg.u32(new.steps), want.steps) and fg.u32(links_out).tobytes() == want.links.tobytes(), (what, r)
    run("flip", seed, one)


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_flatten(seed, tmp_path, monkeypatch):
    def one(k, p, ex, what):
        nm = ex["nm"]
        hook(monkeypatch, FLATTEN_HOOK, ex["chunk"])
        with load(p, tmp_path) as g:
            assert g.flatten_legend().tolist() == flm.legend(p), what
            want = flm.bed(p, nm)
            got = g.flatten_bed(nm)
            assert len(got) == len(want) and got == want, what
            fasta = g.flatten_fasta(nm)
            assert fasta == flm.fasta(p, nm), what
            sizes = []
            g.flatten_stream(nm, 2, lambda b: sizes.append(len(b)))
            n_lines = want.count(b"\n") - 1
            assert sum(sizes) == len(want) and len(sizes) >= 1 + (-(-n_lines // ex["chunk"]) if ex["chunk"] else 1), what
    run("flatten", seed, one)


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_print(seed, tmp_path, monkeypatch):
    def one(k, p, ex, what):
        hook(monkeypatch, PRINT_HOOK, ex["chunk"])
        want = pm.gfa(p)
        with load(p, tmp_path) as g:
            got = g.gfa_text_device()
            assert len(got) == len(want) and got == want, what
            assert g.gfa_text() == want, what
            if k % 2:
                with pa.parse_bytes_device(got) as back:
                    assert parse_shapes.normalized_pools(back) == parse_shapes.normalized_pools(g), what
    run("print", seed, one)


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_validate_and_degree(seed):
    def one(k, p, ex, what):
        g, flat = load_pools(p)
        try:
            if k % 2:
                g.to_device()  # the resident route: the steps are read in place
            want = same(g, p, what)
            assert g.validate_count() == len(tm.validate(p)) == len(want), what
            assert np.array_equal(g.degree(), tm.degree(p)), what
        finally:
            g.close()
            os.unlink(flat)
    run("topology", seed, one)
