"""chop on the GPU (flatgfa_chop, the flatgfa_dev_chop_* entries, `fgfa chop`, FlatGFA.chop, device.chop) against the model
in tests/chop_model.py.  Run with -m gpu."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import chop_model as cm
import pollen_amd as pa
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
CS = [1, 2, 3, 7, 1 << 40]


def parsable():
    out = []
    for path in golden_gfas():
        try:
            g = pa.parse(path)
        except Exception:
            continue
        g.close()
        out.append(path)
    return out


def load_pools(p: fo.Pools):
    fd, path = tempfile.mkstemp(suffix=".flatgfa")
    with os.fdopen(fd, "wb") as f:
        f.write(fo.dump_flatgfa(p))
    return pa.load(path), path


def check_graph(g, c, links, want=None):
    p = cm.pools_of(g)
    if want is None:
        want = cm.chop(p, c, links)
    q = g.chop(c, links)
    got = cm.pools_of(q)
    for n in fo.POOL_ORDER:
        assert getattr(got, n).tobytes() == getattr(want, n).tobytes(), (n, c, links)
    text = q.gfa_text()
    assert text == cm.text(want)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "c.flatgfa")
        q.write_flatgfa(out)
        assert pa.load(out).gfa_text() == text
    return q


@pytest.mark.parametrize("path", parsable(), ids=fixture_id)
def test_golden_graphs_every_c(path):
    g = pa.parse(path)
    for c in CS:
        for links in (False, True):
            check_graph(g, c, links)


@pytest.mark.parametrize("path", parsable(), ids=fixture_id)
def test_cli_bytes(path):
    p = cm.pools_of(pa.parse(path))
    for links in (False, True):
        want = cm.text(cm.chop(p, 3, links))
        r = subprocess.run([FGFA, "-I", path, "chop", "-c", "3"] + (["-l"] if links else []), capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout == want, r.stderr
    with tempfile.TemporaryDirectory() as d:
        flat, txt = os.path.join(d, "o.flatgfa"), os.path.join(d, "o.gfa")
        subprocess.run([FGFA, "-I", path, "-o", flat, "chop", "-c", "2", "-l"], check=True, capture_output=True, timeout=120)
        subprocess.run([FGFA, "-I", path, "-O", txt, "chop", "-c", "2", "-l"], check=True, capture_output=True, timeout=120)
        want = cm.text(cm.chop(p, 2, True))
        assert pa.load(flat).gfa_text() == want
        assert open(txt, "rb").read() == want
        r = subprocess.run([FGFA, "-i", flat, "chop", "-c", "1"], capture_output=True, timeout=120)
        assert r.stdout == cm.text(cm.chop(cm.chop(p, 2, True), 1, False))


def test_flip3_known_cli():
    path = os.path.join(GOLDEN, "ref_handmade_flip3.gfa")
    r = subprocess.run([FGFA, "-I", path, "chop", "-c", "3", "-l"], capture_output=True, check=True, timeout=120)
    q = cm.chop(cm.pools_of(pa.parse(path)), 3, True)
    assert len(q.links) > 20 and r.stdout == cm.text(q)


def random_gfa(seed, n_segs=120, n_paths=8):
    rng = np.random.default_rng(seed)
    names = [int(rng.integers(1, 50)) if i % 9 == 0 else i + 1 for i in range(n_segs)]  # duplicate names too
    lines = [b"H\tVN:Z:1.0"]
    for nm in names:
        lines.append(b"S\t%d\t%s" % (nm, bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, 301))))))
    o = lambda: b"+-"[int(rng.integers(0, 2)):][:1]  # noqa: E731
    for k in range(n_paths):
        n = int(rng.integers(1, 60))  # (the printer, as print.rs, takes no path without steps)
        lines.append(b"P\tp%d\t" % k + b",".join(b"%d%s" % (names[int(rng.integers(0, n_segs))], o()) for _ in range(n)) + b"\t*")
    for _ in range(40):
        a = names[int(rng.integers(0, n_segs))]
        b = a if rng.random() < 0.2 else names[int(rng.integers(0, n_segs))]  # self-loops
        lines.append(b"L\t%d\t%s\t%d\t%s\t0M" % (a, o(), b, o()))
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs(seed):
    g = pa.parse_bytes(random_gfa(seed))
    for c in CS:
        for links in (False, True):
            check_graph(g, c, links)


def test_errors():
    g = pa.parse_bytes(b"S\t1\tACGT\nP\tp\t1+\t*\n")
    with pytest.raises(pa.FlatGFAError) as e:
        g.chop(0)
    assert e.value.code == -1
    p = cm.pools_of(g)
    p.steps = np.array([6], np.uint32)  # segment 3 of 1
    h, path = load_pools(p)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            h.chop(3)
        assert e.value.code == -2
    finally:
        h.close()
        os.unlink(path)
    # 4 097 steps of a 1 Mbp segment at c = 1: 2^32 + 2^20 new steps, refused before any output exists
    big = pa.parse_bytes(b"S\t1\t" + b"A" * (1 << 20) + b"\nP\tp\t" + b",".join([b"1+"] * 4097) + b"\t*\n")
    with pytest.raises(pa.FlatGFAError) as e:
        big.chop(1)
    assert e.value.code == -6
    assert len(cm.pools_of(big.chop(1 << 20)).steps) == 4097
    r = subprocess.run([FGFA, "chop", "-c", "0"], input=b"S\t1\tA\n", capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stdout == b""


def test_device_too_large():
    import torch
    d = torch.device("cuda:0")
    seg_len = torch.tensor([1 << 31], dtype=torch.int64).to(torch.int32).to(d)
    e = torch.zeros(0, dtype=torch.int32, device=d)
    dg = pdev.DeviceGraph.from_tensors(e, e, e, 1, seg_len)
    with pytest.raises(pa.FlatGFAError) as ex:
        pdev.chop(dg, 1)
    assert ex.value.code == -6
    with pytest.raises(pa.FlatGFAError) as ex:
        pdev.chop(pdev.DeviceGraph.from_tensors(e, e, e, 1, None), 1)
    assert ex.value.code == -1


def device_graph_of(p: fo.Pools):
    lens = (p.segs["seq_end"] - p.segs["seq_start"]).astype(np.uint32)
    return pdev.DeviceGraph(p.steps, p.paths["steps_start"], p.paths["steps_end"], len(p.segs), lens)


def check_device(p, c):
    want = cm.chop_fast(p, c)
    dg, sf = pdev.chop(device_graph_of(p), c)
    assert np.array_equal(sf.cpu().numpy().view(np.uint32), cm.seg_first(p, c).astype(np.uint32))
    assert np.array_equal(dg.steps.cpu().numpy().view(np.uint32), want.steps)
    assert np.array_equal(dg.path_begin.cpu().numpy().view(np.uint32), want.paths["steps_start"])
    assert np.array_equal(dg.path_end.cpu().numpy().view(np.uint32), want.paths["steps_end"])
    assert np.array_equal(dg.seg_len.cpu().numpy().view(np.uint32), (want.segs["seq_end"] - want.segs["seq_start"]).astype(np.uint32))
    return dg, sf, want


def test_device_arbitrary_and_overlapping_spans():
    rng = np.random.default_rng(7)
    p = cm.pools_of(pa.parse_bytes(random_gfa(11, n_segs=300, n_paths=40)))
    n = len(p.steps)
    for i in range(len(p.paths)):
        s = int(rng.integers(0, n + 1))
        p.paths[i]["steps_start"], p.paths[i]["steps_end"] = s, int(rng.integers(s, n + 1))
    p.paths[3]["steps_start"], p.paths[3]["steps_end"] = 0, n  # one covering all, over the others
    for c in CS:
        check_device(p, c)


@pytest.mark.parametrize("backward", [False, True])
def test_giant_segments(backward):
    # three multi-Mbp segments at c = 1 among 100 000 short ones, stepped by 4 paths
    rng = np.random.default_rng(3)
    S = 100_003
    lens = rng.integers(1, 33, S).astype(np.int64)
    lens[[5, 50_000, 100_000]] = [5_000_000, 3_000_001, 1_234_567]
    p = synthetic_pools(rng, lens, 4, 40_000, giant=[5, 50_000, 100_000], backward=backward)
    dg, sf, want = check_device(p, 1)
    h, path = load_pools(p)
    try:
        assert np.array_equal(cm.pools_of(h.chop(1)).steps, want.steps)
    finally:
        h.close()
        os.unlink(path)


def synthetic_pools(rng, lens, n_paths, steps_per_path, giant=(), backward=False):
    S = len(lens)
    st = np.concatenate([[0], np.cumsum(lens)[:-1]])
    segs = np.zeros(S, fo.SEG_DT)
    segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, S + 1), st, st + lens
    steps = []
    for k in range(n_paths):
        s = rng.integers(0, S, steps_per_path).astype(np.uint32)
        s[rng.integers(0, steps_per_path, len(giant) * 3)] = np.repeat(np.array(giant, np.uint32), 3)[:len(giant) * 3] if len(giant) else s[:0]
        o = np.ones(steps_per_path, np.uint32) if backward else rng.integers(0, 2, steps_per_path).astype(np.uint32)
        steps.append((s << 1) | o)
    steps = np.concatenate(steps) if steps else np.zeros(0, np.uint32)
    names = b"".join(b"p%d" % k for k in range(n_paths))
    paths = np.zeros(n_paths, fo.PATH_DT)
    off = 0
    for k in range(n_paths):
        ln = len(b"p%d" % k)
        paths[k]["name_start"], paths[k]["name_end"] = off, off + ln
        off += ln
        paths[k]["steps_start"], paths[k]["steps_end"] = k * steps_per_path, (k + 1) * steps_per_path
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=paths, links=np.zeros(0, fo.LINK_DT), steps=steps,
                    seq_data=np.full(int(lens.sum()), ord("A"), np.uint8), overlaps=np.zeros(0, fo.SPAN_DT),
                    alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(names, np.uint8).copy(), optional_data=z, line_order=z)


def test_million_segments_20m_steps():
    g = pa.synth(5, 1_000_000, 20, 1_000_000, "pangenome", False)
    p = cm.pools_of(g)
    for c in (16,):  # (about 30 M new steps: what the numpy model holds in a few GB)
        want = cm.chop_fast(p, c)
        q = cm.pools_of(g.chop(c))
        for n in ("segs", "paths", "steps", "links"):
            assert getattr(q, n).tobytes() == getattr(want, n).tobytes(), (n, c)
    check_device(p, 16)


def test_resident_handle():
    g = pa.synth(2, 5_000, 30, 2_000, "pangenome", True)
    before = cm.pools_of(g.chop(3, True))
    g.to_device()
    d0, u0 = g.seg_depth_with_uniq()
    after = cm.pools_of(g.chop(3, True))
    assert cm.same_pools(before, after)
    d1, u1 = g.seg_depth_with_uniq()
    assert np.array_equal(d0, d1) and np.array_equal(u0, u1)
    assert cm.same_pools(after, cm.chop_fast(cm.pools_of(g), 3, True))


def test_chop_then_depth_on_device():
    import torch
    g = pa.synth(4, 20_000, 12, 30_000, "pangenome", False)
    p = cm.pools_of(g)
    d_old, u_old = fo.seg_depth_with_uniq(p)
    ln_old, _ = fo.path_depth(p)
    dg, sf = pdev.chop(device_graph_of(p), 3)
    S2 = dg.n_segs
    depth = torch.zeros(S2, dtype=torch.int32, device=dg.device)
    uniq = torch.zeros(S2, dtype=torch.int32, device=dg.device)
    plan = pdev.DepthPlan(dg, first=(depth, uniq))
    assert plan.first_status == 0
    sfirst = sf.cpu().numpy().view(np.uint32).astype(np.int64)
    old = np.repeat(np.arange(len(p.segs)), np.diff(sfirst))
    assert np.array_equal(depth.cpu().numpy().view(np.uint32).astype(np.uint64), d_old[old].astype(np.uint64))
    assert np.array_equal(uniq.cpu().numpy().view(np.uint32).astype(np.uint64), u_old[old].astype(np.uint64))
    P = dg.n_paths
    ln = torch.zeros(P, dtype=torch.int64, device=dg.device)
    wt = torch.zeros(P, dtype=torch.int64, device=dg.device)
    plan.path_depth_all(depth, ln, wt)
    torch.cuda.synchronize()
    assert np.array_equal(ln.cpu().numpy().astype(np.uint64), np.asarray(ln_old, dtype=np.uint64))
    plan.close()
