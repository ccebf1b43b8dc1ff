"""flip on the GPU (flatgfa_flip, flatgfa_flip_count, the flatgfa_dev_flip_* pair, `fgfa flip`, FlatGFA.flip, device.flip)
against the model in tests/flip_model.py and the reference's own output in tests/golden/flip.  The reference sorts its lines
and prints its links normalised, so its text is compared by views; the model is compared pool for pool.  Run with -m gpu."""
import json
import os
import subprocess

import numpy as np
import pytest

import crush_model as cm
import flip_gpu as fg
import flip_model as fm
import pollen_amd as pa
from conftest import GOLDEN, ROOT, golden_gfas
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
FLIP = os.path.join(GOLDEN, "flip")
with open(os.path.join(FLIP, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
FIXTURES = golden_gfas() + [os.path.join(FLIP, "synth_flip.gfa.txt")]


def stem_of(path):
    return os.path.basename(path).split(".")[0]


@pytest.fixture(scope="module")
def models():
    """Per fixture: the input's pools and the model's flip of them, made once."""
    out = {}
    for path in FIXTURES:
        g = pa.parse(path)
        p = fm.pools_of(g)
        g.close()
        out[path] = (p, fm.flip(p))
    return out


def test_there_are_14_fixtures_and_seven_turn_a_path(models):
    assert len(FIXTURES) == 14
    assert sum(1 for p, _ in models.values() if fm.turned(p).any()) == 7


@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_handle(path, models):
    p, want = models[path]
    g = pa.parse(path)
    q = g.flip()
    fm.assert_same_pools(fm.pools_of(q), want, "flip")
    fm.assert_same_pools(fm.pools_of(g), p, "the input is only read")
    n_turned, n_links = g.flip_count()
    assert (n_turned, n_links) == (int(fm.turned(p).sum()), len(want.links)) and q.path_count == g.path_count
    assert n_turned == sum(1 for a, b in zip(fm.new_names(p, fm.turned(p)), fm.new_names(p, np.zeros(len(p.paths), bool))) if a != b)
    text = q.gfa_text()
    assert text == fm.text(want)
    rec = MANIFEST[stem_of(path) + ".flip.gfa.txt"]
    if rec["input_ends_in_newline"]:
        with open(os.path.join(FLIP, stem_of(path) + ".flip.gfa.txt"), "rb") as f:
            ref = cm.text_views(f.read())
        for a, b, what in zip(cm.text_views(text, ours=True), ref, "SPLH"):
            assert a == b, what
        assert (n_turned, len(p.links), n_links) == (rec["turned"], rec["links_in"], rec["links_out"])
    # flip of flip: nothing turns twice and the links are unique already -- equal pools; and the new handle outlives the old
    g.close()
    assert q.flip_count() == (0, len(want.links))
    qq = q.flip()
    fm.assert_same_pools(fm.pools_of(qq), want, "flip of flip")
    q.close()
    assert qq.gfa_text() == text
    qq.close()


@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_validate_accepts_every_turned_path(path, models):
    p, want = models[path]
    t = fm.turned(p)
    g = pa.parse(path)
    q = g.flip()
    missing = q.validate()
    assert not np.isin(missing["path"], np.flatnonzero(t)).any()
    # a path that stayed misses nothing it did not miss before: flip drops no class of links
    before = {r.tobytes() for r in g.validate()}
    assert all(r.tobytes() in before for r in missing)
    q.close()
    g.close()


@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_cli_text_and_flatgfa(path, models, tmp_path):
    p, want = models[path]
    r = subprocess.run([FGFA, "-I", path, "flip"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == fm.text(want), r.stderr
    flat = str(tmp_path / "o.flatgfa")
    subprocess.run([FGFA, "-I", path, "-o", flat, "flip"], check=True, capture_output=True, timeout=120)
    h = pa.load(flat)
    fm.assert_same_pools(fm.pools_of(h), want, "-o")
    h.close()
    r = subprocess.run([FGFA, "-i", flat, "flip"], capture_output=True, timeout=120)  # flip of flip, from the file
    assert r.returncode == 0 and r.stdout == fm.text(want), r.stderr


def test_cli_usage_error_exits_2(tmp_path):
    r = subprocess.run([FGFA, "-I", os.path.join(GOLDEN, "ref_tiny.gfa"), "flip", "-x"], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"usage: fgfa flip" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_device_pair(path, models):
    import torch
    p, want = models[path]
    new, links_out, turned = fg.check_device_pair(p, want, what=path)
    # flip of flip on the device: nothing turns, every link stays
    align = torch.from_numpy(np.ascontiguousarray(want.alignment, dtype=np.uint32).view(np.int32).copy()).to(new.device)
    again, links2, turned2 = pdev.flip(new, links_out, alignment=align)
    assert not fg.u32(turned2).any() and np.array_equal(fg.u32(again.steps), want.steps)
    assert fg.u32(links2).tobytes() == want.links.tobytes()


def test_resident_handle_reads_its_steps_in_place(models):
    path = os.path.join(FLIP, "synth_flip.gfa.txt")
    p, want = models[path]
    g = pa.parse(path)
    fm.assert_same_pools(fm.pools_of(g.flip()), want, "a copy of the steps made for the call")
    g.to_device()
    d0 = g.seg_depth()
    fm.assert_same_pools(fm.pools_of(g.flip()), want, "resident")
    assert g.flip_count() == (int(fm.turned(p).sum()), len(want.links))
    assert np.array_equal(g.seg_depth(), d0)
    g.close()


@pytest.mark.parametrize("path", FIXTURES, ids=stem_of)
def test_depths_of_the_flipped_image_are_the_old_ones_on_the_device(path, models):
    """Node depth and unique depth do not see orientation or order: flip(G)'s equal G's bit for bit, the flipped image going
    from device.flip into a DepthPlan with no host copy in between."""
    import torch
    p, want = models[path]
    dg, links, align = fg.to_device(p)
    S = dg.n_segs
    old_d, old_u, new_d, new_u = (torch.zeros(S, dtype=torch.int32, device=dg.device) for _ in range(4))
    plan = pdev.DepthPlan(dg)
    plan.seg_depth(old_d, old_u)
    plan.status()
    new, _, _ = pdev.flip(dg, links, alignment=align)
    plan2 = pdev.DepthPlan(new)
    plan2.seg_depth(new_d, new_u)
    plan2.status()
    torch.cuda.synchronize()
    assert torch.equal(old_d, new_d) and torch.equal(old_u, new_u)
    assert S == 0 or len(p.steps) == 0 or int(old_d.sum()) > 0
    plan.close()
    plan2.close()
