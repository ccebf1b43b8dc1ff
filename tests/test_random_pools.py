"""tests/random_pools.py on the CPU, for every seed and case that tests/test_gpu_random_slices.py runs: the pools are legal, the
two forms of each feature's model agree on them, the model's output keeps the feature's invariant, and the census of the
classes each case reaches (random_pools.CLASSES, from the pools and the kernels' constants) meets its conditions -- every
class in at least 20 cases of its feature's slice and in every seed, no case skipped.  No GPU."""
import numpy as np
import pytest

import crush_model as cm
import flatten_model as flm
import flip_model as fm
import pollen_amd as pa
import print_model as pm
import random_pools as rp
import topology_model as tm
from oracle import flatgfa_oracle as fo

FEATURES = list(rp.CASES)
BY_SEED = [(f, s) for f in FEATURES for s in rp.SEEDS]
MIN_CASES = 20


def cases(feature, seed):
    for k in range(rp.CASES[feature]):
        sd = rp.case_seed(seed, k)
        yield sd, rp.make(sd, feature)


def test_the_constants_are_the_sources():
    assert rp.C["crush"]["TILE"] == cm.TILE and rp.CRUSH_STEP * (rp.CRUSH_QUARTER // rp.CRUSH_STEP) == rp.CRUSH_QUARTER
    assert rp.CRUSH_QUARTER * (cm.THREADS // rp.WAVE) == cm.TILE
    assert (rp.SHORT_ROW, rp.LDS_ROW, rp.LONG_NAME, rp.TEXT_TILE) == (fm.SHORT_ROW, fm.LDS_ROW, flm.LONG_NAME, flm.TILE)


def test_make_is_deterministic():
    for f in FEATURES + ["text"]:
        a, b = rp.make(rp.case_seed(3, 4), f), rp.make(rp.case_seed(3, 4), f)
        cm.assert_same_pools(a, b, f)
        assert any(getattr(a, n).tobytes() != getattr(rp.make(rp.case_seed(3, 5), f), n).tobytes() for n in fo.POOL_ORDER)


@pytest.mark.parametrize("feature", FEATURES)
def test_census(feature):
    """Every class in at least MIN_CASES cases of the slice and in every seed."""
    in_cases = {c: 0 for c in rp.CLASSES[feature]}
    total = dict(in_cases)
    n = 0
    for seed in rp.SEEDS:
        of_seed = {c: 0 for c in rp.CLASSES[feature]}
        for k in range(rp.CASES[feature]):
            cen = rp.case_census(rp.case_seed(seed, k), feature)
            assert list(cen) == rp.CLASSES[feature]
            n += 1
            for c, v in cen.items():
                of_seed[c] += v
                total[c] += v
                in_cases[c] += v > 0
        assert all(of_seed.values()), (feature, seed, of_seed)
    print(feature, n, "cases;", "; ".join("%s: %d cases, %d instances" % (c, in_cases[c], total[c]) for c in in_cases))
    assert n == len(rp.SEEDS) * rp.CASES[feature] and 30 <= rp.CASES[feature] <= 50
    assert all(v >= MIN_CASES for v in in_cases.values()), in_cases


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_crush(seed):
    for sd, p in cases("crush", seed):
        fm.check(p)
        a, b = cm.crush(p), cm.crush_fast(p)
        cm.assert_same_pools(a, b, sd)
        data = b.seq_data.tobytes()
        for s in b.segs:  # no NN inside a segment
            assert b"NN" not in data[int(s["seq_start"]):int(s["seq_end"])], sd
        assert cm.dropped(p) > 0 and cm.dropped(b) == 0


def pairs_of(st):
    return {(int(a), int(b)) for a, b in zip(st[:-1], st[1:])}


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_flip(seed):
    for sd, p in cases("flip", seed):
        fm.check(p)
        q = fm.flip(p)
        fm.assert_same_pools(fm.flip(p, fast=False), q, sd)
        have = set(zip(q.links["from_"].tolist(), q.links["to"].tolist()))
        t = fm.turned(p)
        for i in np.flatnonzero(t).tolist():  # every consecutive pair of a turned path's new steps is a link, in one spelling
            for a, b in pairs_of(fm.path_steps(q, i)):
                assert (a, b) in have or (b ^ 1, a ^ 1) in have, (sd, i, a, b)
        assert not fm.turned(q).any()


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_topology(seed):
    for sd, p in cases("topology", seed):
        fm.check(p)
        have = set(zip(p.links["from_"].tolist(), p.links["to"].tolist()))
        want = []
        for i, path in enumerate(p.paths):  # a plain set lookup, not the model's sorted keys
            st = p.steps[int(path["steps_start"]):int(path["steps_end"])].tolist()
            want += [(i, j, a, b) for j, (a, b) in enumerate(zip(st[:-1], st[1:])) if (a, b) not in have and (b ^ 1, a ^ 1) not in have]
        got = tm.validate(p)
        assert [tuple(int(x) for x in r) for r in got] == want, sd
        deg = [0] * len(p.segs)
        for a, b in zip(p.links["from_"].tolist(), p.links["to"].tolist()):
            deg[a >> 1] += 1
            deg[b >> 1] += 1
        assert tm.degree(p).tolist() == deg, sd


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_flatten(seed):
    for sd, p in cases("flatten", seed):
        fm.check(p)
        nm = rp.extras(sd, "flatten")["nm"]
        bed = flm.bed(p, nm)
        assert flm.bed_fast(p, nm) == bed, sd
        assert bed.count(b"\n") == 1 + int((p.paths["steps_end"].astype(np.int64) - p.paths["steps_start"]).sum())
        body = flm.fasta(p, nm)[len(nm) + 2:]
        assert len(body) == flm.fasta_body_len(flm.legend(p)[-1]) and body.replace(b"\n", b"") == flm.bases(p), sd


@pytest.mark.parametrize("seed", rp.SEEDS)
def test_print(seed, tmp_path):
    for sd, p in cases("print", seed):
        fm.check(p)
        f = tmp_path / "case.flatgfa"
        f.write_bytes(fo.dump_flatgfa(p))
        with pa.load(str(f)) as g:  # the host printer is the model's second opinion
            text = g.gfa_text()
        assert text == pm.gfa(p), sd
        assert text.count(b"\n") == len(p.segs) + len(p.paths) + len(p.links) + (1 if len(p.header) else 0), sd


@pytest.mark.parametrize("seed", rp.TEXT_SEEDS)
def test_text_profile_is_what_the_reference_reads(seed):
    p = rp.make(seed, "text")
    fm.check(p)
    assert len(p.segs) <= 300 and len(p.steps) <= 2000
    lens = p.segs["seq_end"].astype(np.int64) - p.segs["seq_start"]
    assert (lens > 0).all() and np.array_equal(p.segs["seq_start"][1:], p.segs["seq_end"][:-1]) and set(p.seq_data.tolist()) <= set(b"ACGTN")
    assert (p.paths["steps_end"] > p.paths["steps_start"]).all() and len({p.path_name(i) for i in range(len(p.paths))}) == len(p.paths)
    q = fo.parse_gfa(rp.gfa_text(p))  # the text says the pools
    for n in ("segs", "steps", "seq_data", "name_data", "header"):
        assert getattr(q, n).tobytes() == getattr(p, n).tobytes(), n
    assert q.links["from_"].tolist() == p.links["from_"].tolist() and q.links["to"].tolist() == p.links["to"].tolist()
    # what the goldens lacked: N on both sides of a seam, a tie, a palindrome, a self-loop, a row past the linear probe
    assert cm.dropped(p) > 20 and any(f == r and f for f, r in (fm.weigh(p, i) for i in range(len(p.paths))))
    lk = set(zip(p.links["from_"].tolist(), p.links["to"].tolist()))
    assert any(a == b ^ 1 for a, b in lk) and any(a == b for a, b in lk)
    assert int(np.bincount(p.links["from_"]).max()) > rp.TOPO_LINEAR
