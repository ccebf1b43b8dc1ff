"""crush on the GPU (flatgfa_crush, the flatgfa_dev_crush_* pair, `fgfa crush`, FlatGFA.crush, device.crush) against the model
in tests/crush_model.py and the reference's own output in tests/golden/crush.  Run with -m gpu."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import crush_gpu as cg
import crush_model as cm
import pollen_amd as pa
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
CRUSH = os.path.join(GOLDEN, "crush")
with open(os.path.join(CRUSH, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
FIXTURES = golden_gfas() + [os.path.join(CRUSH, "synth_crush.gfa")]


@pytest.fixture(scope="module")
def models():
    """Per fixture: the input's pools and the model's crush of them, made once."""
    out = {}
    for path in FIXTURES:
        g = pa.parse(path)
        p = cm.pools_of(g)
        g.close()
        out[path] = (p, cm.crush(p))
    return out


def test_there_are_14_fixtures_and_two_drop_bytes(models):
    assert len(FIXTURES) == 14
    assert sum(1 for p, _ in models.values() if cm.dropped(p) > 0) >= 2


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_handle(path, models):
    p, want = models[path]
    g = pa.parse(path)
    q = g.crush()
    cm.assert_same_pools(cm.pools_of(q), want, "crush")
    cm.assert_same_pools(cm.pools_of(g), p, "the input is only read")
    text = q.gfa_text()
    assert text == cm.text(want)
    rec = MANIFEST[fixture_id(path) + ".crush.gfa"]
    if rec["input_ends_in_newline"]:
        with open(os.path.join(CRUSH, fixture_id(path) + ".crush.gfa"), "rb") as f:
            ref = cm.text_views(f.read())
        for a, b, what in zip(cm.text_views(text, ours=True), ref, "SPLH"):
            assert a == b, what
        assert cm.dropped(p) == rec["dropped"]
    # crush of crush: nothing dropped, equal pools; and the new handle outlives the old
    g.close()
    qq = q.crush()
    cm.assert_same_pools(cm.pools_of(qq), want, "crush of crush")
    assert len(cm.pools_of(qq).seq_data) == len(want.seq_data)
    q.close()
    assert qq.gfa_text() == text
    qq.close()


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_cli_text_and_flatgfa(path, models, tmp_path):
    p, want = models[path]
    r = subprocess.run([FGFA, "-I", path, "crush"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == cm.text(want), r.stderr
    flat = str(tmp_path / "o.flatgfa")
    subprocess.run([FGFA, "-I", path, "-o", flat, "crush"], check=True, capture_output=True, timeout=120)
    h = pa.load(flat)
    cm.assert_same_pools(cm.pools_of(h), want, "-o")
    h.close()
    r = subprocess.run([FGFA, "-i", flat, "crush"], capture_output=True, timeout=120)  # crush of crush, from the file
    assert r.returncode == 0 and r.stdout == cm.text(want), r.stderr


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_device_pair(path, models):
    p, want = models[path]
    new, seq_out, seg_seq_out = cg.check_device_pair(p, want, what=path)
    # crush of crush on the device: 0 dropped, equal pools
    again, seq2, spans2 = pdev.crush(new, seg_seq_out, seq_out)
    assert seq2.numel() == seq_out.numel() and bytes(seq2.cpu().numpy()) == want.seq_data.tobytes()
    assert np.array_equal(cg.u32(spans2), cg.u32(seg_seq_out)) and np.array_equal(cg.u32(again.seg_len), cg.u32(new.seg_len))


def test_resident_handle_and_its_device_pool(models):
    path = os.path.join(CRUSH, "synth_crush.gfa")
    p, want = models[path]
    g = pa.parse(path)
    cm.assert_same_pools(cm.pools_of(g.crush()), want, "a copy of the pool made for the call")
    g.to_device()
    d0 = g.seg_depth()
    cm.assert_same_pools(cm.pools_of(g.crush()), want, "resident")
    fasta = g.flatten_fasta(b"x")  # (leaves the sequence pool on the device with the handle)
    cm.assert_same_pools(cm.pools_of(g.crush()), want, "the handle's device pool")
    assert g.flatten_fasta(b"x") == fasta and np.array_equal(g.seg_depth(), d0)
    g.close()


def test_crush_then_path_depth_and_legend_stay_on_the_device(models):
    import torch
    path = os.path.join(CRUSH, "synth_crush.gfa")
    p, want = models[path]
    new, _, _ = cg.check_device_pair(p, want)
    S, P = new.n_segs, new.n_paths
    depth = torch.zeros(S, dtype=torch.int32, device=new.device)
    ln = torch.zeros(P, dtype=torch.int64, device=new.device)
    wt = torch.zeros(P, dtype=torch.int64, device=new.device)
    plan = pdev.DepthPlan(new)
    plan.path_depth_all(depth, ln, wt)
    plan.status()
    torch.cuda.synchronize()
    want_ln, want_mean = fo.path_depth(want)
    old_ln, _ = fo.path_depth(p)
    assert np.array_equal(ln.cpu().numpy().astype(np.uint64), np.asarray(want_ln, dtype=np.uint64))
    assert not np.array_equal(np.asarray(want_ln), np.asarray(old_ln))  # (the paths walk crushed segments)
    mean = wt.cpu().numpy().astype(np.uint64).astype(np.float64) / np.asarray(want_ln, dtype=np.float64)
    assert np.allclose(mean, want_mean, rtol=1e-12)
    plan.close()
    legend = torch.zeros(S + 1, dtype=torch.int64, device=new.device)
    g = new.c_struct()
    assert _lib.lib().flatgfa_dev_flatten_legend(ctypes.byref(g), legend.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert legend.cpu().numpy().tolist() == [0] + np.cumsum(want.segs["seq_end"].astype(np.int64) - want.segs["seq_start"]).tolist()
