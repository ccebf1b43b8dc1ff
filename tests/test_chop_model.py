"""The chop model (tests/chop_model.py) against slow_odgi's goldens and hand-worked answers, its numpy form against it, and
the argument checks of the C ABI and the CLI that need no device."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import chop_model as cm
from conftest import GOLDEN, ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

CHOP = os.path.join(GOLDEN, "chop")
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def parse(text: bytes) -> fo.Pools:
    return fo.parse_gfa(text)


def goldens():
    return sorted(glob.glob(os.path.join(CHOP, "*.chop3.gfa")))


def test_goldens_exist():
    assert len(goldens()) >= 10


@pytest.mark.parametrize("golden", goldens(), ids=lambda p: os.path.basename(p)[:-10])
def test_model_matches_slow_odgi(golden):
    src = os.path.join(GOLDEN, os.path.basename(golden)[:-len(".chop3.gfa")] + ".gfa")
    with open(src, "rb") as f:
        p = parse(f.read())
    with open(golden, "rb") as f:
        want = cm.parse_odgi_text(f.read())
    # slow_odgi drops links (chop.py:67): segments and paths only
    for links in (False, True):
        assert cm.odgi_view(cm.chop(p, 3, links)) == want


def test_atggccc_at_2():
    # slow_odgi/chop.py:18-27: S 3 = ATGGCCC at n = 2 becomes AT, GG, CC, C
    p = parse(b"S\t3\tATGGCCC\nP\tp\t3+\t*\n")
    q = cm.chop(p, 2)
    segs, paths = cm.odgi_view(q)
    assert segs == {"1": "AT", "2": "GG", "3": "CC", "4": "C"}
    assert paths == {"p": ["1+", "2+", "3+", "4+"]}
    assert cm.text(q) == b"S\t1\tAT\nS\t2\tGG\nS\t3\tCC\nS\t4\tC\nP\tp\t1+,2+,3+,4+\t*\n"


def test_backward_steps_come_out_reversed():
    p = parse(b"S\t1\tACGTACG\nS\t2\tTT\nP\tp\t1-,2+,1+\t*\n")
    q = cm.chop(p, 3)
    assert q.steps.tolist() == [(2 << 1) | 1, (1 << 1) | 1, (0 << 1) | 1, 3 << 1, 0, 2, 4]
    assert cm.odgi_view(q)[1] == {"p": ["3-", "2-", "1-", "4+", "1+", "2+", "3+"]}


def test_links_every_orientation_pair():
    # a (5 bp -> 2 pieces at c = 3), b (7 bp -> 3 pieces), c (2 bp -> kept)
    p = parse(b"S\t1\tAAAAA\nS\t2\tCCCCCCC\nS\t3\tGG\nL\t1\t+\t2\t+\t0M\nL\t1\t-\t2\t-\t0M\nL\t1\t+\t2\t-\t0M\n"
              b"L\t1\t-\t2\t+\t0M\nL\t3\t+\t3\t-\t0M\nP\tp\t1+,2-\t*\n")
    q = cm.chop(p, 3, links=True)
    # new ids: a -> 0, 1; b -> 2, 3, 4; c -> 5
    fw = [(0, 0, 1, 0), (2, 0, 3, 0), (3, 0, 4, 0)]  # chop.rs:14-22, in segment order
    old = [(1, 0, 2, 0),   # 1+ -> 2+: from the last piece of a, to the first of b
           (0, 1, 4, 1),   # 1- -> 2-: from the first of a, to the last of b
           (1, 0, 4, 1),   # 1+ -> 2-
           (0, 1, 2, 0),   # 1- -> 2+
           (5, 0, 5, 1)]   # a self-loop of a segment that stays whole
    got = [(int(l["from_"]) >> 1, int(l["from_"]) & 1, int(l["to"]) >> 1, int(l["to"]) & 1) for l in q.links]
    assert got == fw + old
    assert (q.links["ov_start"] == 0).all() and (q.links["ov_end"] == 0).all()
    assert cm.chop(p, 3, links=False).links.size == 0
    t = cm.text(q)
    assert t.index(b"\nP\t") < t.index(b"\nL\t")  # normalized order: H, S, P, L


@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_lengths_0_c_c1_kc(c):
    seqs = [b"", b"A" * c, b"C" * (c + 1), b"G" * (3 * c)]
    p = parse(b"".join(b"S\t%d\t%s\n" % (i + 1, s) for i, s in enumerate(seqs)) + b"P\tp\t1+,2+,3-,4+\t*\n")
    lens = p.segs["seq_end"] - p.segs["seq_start"]
    assert lens.tolist() == [0, c, c + 1, 3 * c]
    q = cm.chop(p, c)
    k = [1, 1, 2, 3]  # length 0 stays one segment (chop.rs:27), c one, c + 1 two, k * c exactly k
    assert len(q.segs) == sum(k)
    assert (q.segs["seq_end"] - q.segs["seq_start"]).tolist() == [0, c, c, 1, c, c, c]
    assert q.segs["name"].tolist() == list(range(1, 8))
    assert cm.seg_first(p, c).tolist() == [0, 1, 2, 4, 7]
    assert q.steps.tolist() == [0, 2, (3 << 1) | 1, (2 << 1) | 1, 8, 10, 12]


def test_empty_paths_and_no_paths():
    p = parse(b"S\t1\tACGTA\nP\te\t\t*\nP\tq\t1+\t*\nP\tf\t\t*\n")
    q = cm.chop(p, 2)
    assert [(int(x["steps_start"]), int(x["steps_end"])) for x in q.paths] == [(0, 0), (0, 3), (3, 3)]
    assert (q.paths["ov_start"] == 0).all() and (q.paths["ov_end"] == 0).all()
    r = cm.chop(parse(b"S\t1\tACGTA\n"), 2)
    assert len(r.segs) == 3 and r.steps.size == 0 and r.paths.size == 0


def test_model_errors():
    p = parse(b"S\t1\tACGTA\nP\tq\t1+\t*\n")
    with pytest.raises(ValueError):
        cm.chop(p, 0)
    p.steps = np.array([4], np.uint32)
    with pytest.raises(IndexError):
        cm.chop(p, 2)
    with pytest.raises(IndexError):
        cm.chop_fast(p, 2)


def random_pools(seed, n_segs=60, n_paths=6, tiling=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 40, n_segs)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(n))) for n in lens]
    names = [int(rng.integers(1, 30)) if i % 7 == 0 else i + 1 for i in range(n_segs)]  # (some repeat)
    lines = [b"S\t%d\t%s" % (nm, s) for nm, s in zip(names, seqs)]
    for k in range(n_paths):
        n = int(rng.integers(0, 30))
        lines.append(b"P\tp%d\t" % k + b",".join(b"%d%s" % (names[int(rng.integers(0, n_segs))], b"+-"[int(rng.integers(0, 2)):][:1]) for _ in range(n)) + b"\t*")
    for _ in range(20):
        a, b = (names[int(i)] for i in rng.integers(0, n_segs, 2))
        lines.append(b"L\t%d\t%s\t%d\t%s\t0M" % (a, b"+-"[int(rng.integers(0, 2)):][:1], b, b"+-"[int(rng.integers(0, 2)):][:1]))
    p = parse(b"\n".join(lines) + b"\n")
    if not tiling:  # spans that overlap and leave steps out
        n = len(p.steps)
        for i in range(len(p.paths)):
            s = int(rng.integers(0, n + 1))
            p.paths[i]["steps_start"], p.paths[i]["steps_end"] = s, int(rng.integers(s, n + 1))
    return p


@pytest.mark.parametrize("seed", range(12))
def test_fast_model_equals_model(seed):
    p = random_pools(seed, tiling=seed % 3 != 0)
    for c in (1, 2, 3, 7, 1 << 40):
        for links in (False, True):
            assert cm.same_pools(cm.chop_fast(p, c, links), cm.chop(p, c, links))


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    out = ctypes.c_void_p(1)
    assert L.flatgfa_chop(None, 3, 0, ctypes.byref(out)) == -1 and out.value is None
    import pollen_amd as pa
    g = pa.parse_bytes(b"S\t1\tACGT\nP\tp\t1+\t*\n")
    assert L.flatgfa_chop(g._h, 0, 0, ctypes.byref(out)) == -1  # c = 0: where the reference loops forever
    assert L.flatgfa_chop(g._h, 3, 0, None) == -1
    job = ctypes.c_void_p()
    n1, n2 = ctypes.c_uint64(), ctypes.c_uint64()
    dg = _lib.flatgfa_dev_graph_t(None, 0, None, None, 0, 1, None)  # seg_len NULL
    assert L.flatgfa_dev_chop_count(ctypes.byref(dg), 3, None, None, ctypes.byref(job), ctypes.byref(n1), ctypes.byref(n2)) == -1
    assert job.value is None


def test_cli_usage_without_c():
    src = os.path.join(GOLDEN, "ref_tiny.gfa")
    for args in ([], ["-c", "0"], ["-c"], ["-c", "x3"], ["-l"], ["-c", "3", "-q"]):
        r = subprocess.run([FGFA, "-I", src, "chop"] + args, capture_output=True, timeout=120)
        assert r.returncode == 2 and r.stdout == b"" and b"usage" in r.stderr, args
