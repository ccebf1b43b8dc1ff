"""inject on the GPU (flatgfa_inject, flatgfa_inject_bed, the flatgfa_dev_inject_* entries, `fgfa inject`, FlatGFA.inject,
device.inject) against the reference's own output (tests/golden/inject/) and the model in tests/inject_model.py.
Run with -m gpu."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import inject_model as im
import pollen_amd as pa
from conftest import GOLDEN, ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
HERE = os.path.join(GOLDEN, "inject")
MANIFEST = json.load(open(os.path.join(HERE, "MANIFEST.json")))
FIXTURES = sorted(os.path.basename(p)[:-len(".inject.bed")] for p in glob.glob(os.path.join(HERE, "*.inject.bed")))


def graph_path(stem):
    return os.path.join(HERE if stem == "synth_inject" else GOLDEN, stem + ".gfa")


def bed_of(stem):
    return open(os.path.join(HERE, stem + ".inject.bed"), "rb").read()


def lines_of(bed):
    return [(f[0], int(f[1]), int(f[2]), f[3]) for f in (ln.split(b"\t") for ln in bed.splitlines() if ln and not ln.startswith(b"#"))]


def s_and_p(text):
    """The H lines in order, and the S lines and the P lines, each sorted (slow_odgi prints both in string order of their
    names, this project in id and path order -- the order is the model's to pin), each line byte for byte.  Nothing else may
    be in either text."""
    ls = [ln for ln in text.split(b"\n") if ln]
    assert all(ln[:2] in (b"H\t", b"S\t", b"P\t") for ln in ls)
    return [ln for ln in ls if ln.startswith(b"H\t")], sorted(ln for ln in ls if ln.startswith(b"S\t")), sorted(ln for ln in ls if ln.startswith(b"P\t"))


def test_there_are_goldens():
    assert len(FIXTURES) == 13 and "synth_inject" in FIXTURES and "edge_names_loops" in MANIFEST["left_out"]
    assert sum(MANIFEST[s]["cuts"] > 0 for s in FIXTURES) >= 11


@pytest.mark.parametrize("stem", FIXTURES)
def test_goldens_through_the_handle(stem):
    want = open(os.path.join(HERE, stem + ".inject.gfa"), "rb").read()
    g = pa.parse(graph_path(stem))
    bed = bed_of(stem)
    q = g.inject(bed)
    assert s_and_p(q.gfa_text()) == s_and_p(want)
    assert q.segment_count - g.segment_count == MANIFEST[stem]["cuts"]
    # the list form, and every pool against the model
    q2 = g.inject([(a.decode(), b, c, d) for a, b, c, d in lines_of(bed)])
    model = im.inject(im.pools_of(g), lines_of(bed))
    for n in fo.POOL_ORDER:
        assert getattr(im.pools_of(q), n).tobytes() == getattr(model, n).tobytes(), n
        assert getattr(im.pools_of(q2), n).tobytes() == getattr(model, n).tobytes(), n


@pytest.mark.parametrize("stem", FIXTURES)
def test_goldens_through_the_cli(stem, tmp_path):
    want = open(os.path.join(HERE, stem + ".inject.gfa"), "rb").read()
    bed = os.path.join(HERE, stem + ".inject.bed")
    r = subprocess.run([FGFA, "-I", graph_path(stem), "inject", "-b", bed], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert s_and_p(r.stdout) == s_and_p(want)
    kinds = [ln[:1] for ln in r.stdout.splitlines()]
    assert b"L" not in kinds and kinds == sorted(kinds, key=b"HSPL".index)  # H, S, P; no links without -l
    # -l against the model, as text and through -o
    g = pa.parse(graph_path(stem))
    model = im.inject(im.pools_of(g), lines_of(bed_of(stem)), links=True)
    r = subprocess.run([FGFA, "-I", graph_path(stem), "inject", "--bed", bed, "-l"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == im.text(model), r.stderr
    flat = str(tmp_path / "o.flatgfa")
    subprocess.run([FGFA, "-I", graph_path(stem), "-o", flat, "inject", "-b", bed, "-l"], check=True, capture_output=True, timeout=120)
    assert im.same_pools(im.pools_of(pa.load(flat)), model)


@pytest.mark.parametrize("stem", ["ref_tiny", "ref_ex2", "ref_handmade_crush1", "standin_k", "standin_note5"])
def test_the_result_validates_when_the_input_did(stem):
    g = pa.parse(graph_path(stem))
    assert len(g.validate()) == 0  # (the fixture is one whose paths are walks of its links)
    bed = bed_of(stem)
    assert MANIFEST[stem]["cuts"] > 0
    q = g.inject(bed, links=True)
    assert q.segment_count > g.segment_count and q.path_count == g.path_count + MANIFEST[stem]["paths_added"]
    assert len(q.validate()) == 0  # old paths over the forward and the remapped links, new paths over the same
    # and without -l there is no link, so every pair of consecutive steps is unsupported
    bare = g.inject(bed)
    paths = im.pools_of(bare).paths
    pairs = int(np.maximum(paths["steps_end"].astype(np.int64) - paths["steps_start"] - 1, 0).sum())
    assert len(bare.validate()) == pairs


@pytest.mark.parametrize("stem", ["synth_inject", "ref_handmade_flip3", "kat_slow_odgi_readme"])
def test_links_resident_and_validate(stem):
    g = pa.parse(graph_path(stem))
    lines = lines_of(bed_of(stem))
    model = im.inject(im.pools_of(g), lines, links=True)
    before = g.inject(bed_of(stem), links=True)
    assert im.same_pools(im.pools_of(before), model)
    g.to_device()
    d0 = g.seg_depth()
    after = g.inject(bed_of(stem), links=True)
    assert im.same_pools(im.pools_of(after), im.pools_of(before))  # resident and non-resident: equal bytes
    assert np.array_equal(g.seg_depth(), d0)  # (the resident image was only read)
    import topology_model as tm
    assert len(after.validate()) == len(tm.validate(model))  # (none of these three validates clean before; the rule itself is below)


@pytest.mark.parametrize("stem", ["synth_inject", "ref_tiny"])
def test_zero_lines_give_the_input(stem):
    g = pa.parse(graph_path(stem))
    p = im.pools_of(g)
    for bed in (b"", b"# nothing\n", b"no_such_path\t1\t2\tx\n"):
        q = im.pools_of(g.inject(bed, links=True))
        assert q.steps.tobytes() == p.steps.tobytes() and q.name_data.tobytes() == p.name_data.tobytes()
        assert np.array_equal(q.segs["seq_start"], p.segs["seq_start"]) and np.array_equal(q.segs["seq_end"], p.segs["seq_end"])
        assert np.array_equal(q.paths["steps_start"], p.paths["steps_start"]) and np.array_equal(q.paths["steps_end"], p.paths["steps_end"])
        assert np.array_equal(q.links["from_"], p.links["from_"]) and np.array_equal(q.links["to"], p.links["to"])
    assert im.same_pools(im.pools_of(g.inject([])), im.inject(p, []))


def test_inject_then_depth_on_the_device():
    import torch
    g = pa.parse(graph_path("synth_inject"))
    p = im.pools_of(g)
    lines = lines_of(bed_of("synth_inject"))
    dev = torch.device("cuda:0")
    ids = torch.tensor([fo.find_path(p, ln[0]) for ln in lines], dtype=torch.int32, device=dev)
    lo = torch.tensor([ln[1] for ln in lines], dtype=torch.int64, device=dev)
    hi = torch.tensor([ln[2] for ln in lines], dtype=torch.int64, device=dev)
    lens = (p.segs["seq_end"] - p.segs["seq_start"]).astype(np.uint32)
    dg, sf = pdev.inject(pdev.DeviceGraph(p.steps, p.paths["steps_start"], p.paths["steps_end"], len(p.segs), lens), ids, lo, hi)
    model = im.inject(p, lines)
    assert np.array_equal(sf.cpu().numpy().view(np.uint32), im.seg_first(p, lines).astype(np.uint32))
    assert np.array_equal(dg.steps.cpu().numpy().view(np.uint32), model.steps)
    assert np.array_equal(dg.path_begin.cpu().numpy().view(np.uint32), model.paths["steps_start"])
    assert np.array_equal(dg.path_end.cpu().numpy().view(np.uint32), model.paths["steps_end"])
    depth = torch.zeros(dg.n_segs, dtype=torch.int32, device=dev)
    uniq = torch.zeros(dg.n_segs, dtype=torch.int32, device=dev)
    plan = pdev.DepthPlan(dg, first=(depth, uniq))
    assert plan.first_status == 0
    again = pa.parse_bytes(g.inject(bed_of("synth_inject")).gfa_text())  # the depth of the re-parsed text
    d, u = fo.seg_depth_with_uniq(im.pools_of(again))
    assert np.array_equal(depth.cpu().numpy().view(np.uint32).astype(np.uint64), d.astype(np.uint64))
    assert np.array_equal(uniq.cpu().numpy().view(np.uint32).astype(np.uint64), u.astype(np.uint64))
    plan.close()


def test_refusals_with_a_device():
    g = pa.parse(graph_path("ref_tiny"))
    for bed in (b"one\t1\t5\ttwo\n", b"one\t1\t5\tx\ntwo\t0\t3\tx\n", b"one\t4\t9\tx\nx\t1\t2\ty\n", b"one\t1\n"):
        with pytest.raises(pa.FlatGFAError) as e:
            g.inject(bed)
        assert e.value.code == -1
    assert im.same_pools(im.pools_of(g.inject(b"one\t1\t5\tx\n")), im.inject(im.pools_of(g), [(b"one", 1, 5, b"x")]))
