"""What a depth plan says of itself (`describe()`) tied to what its calls launch (the per-launch profile's names), at the five
shapes where the call's decisions (pollen_amd/csrc/depth_call_host.hpp: decide_call, scan_mode) take different turns, over
8192 segments each:

  tiny         64 paths of 100 steps: single waves hold them whole (k_scan_tiny), k_scan has nothing to do and is left out
  short        64 paths of 1000 steps: single waves walk them (k_scan_short), likewise
  long         one path of 40 000 steps in runs of 16 ids: an item of k_scan, few enough records for its narrow build
               (emit=two_chunks: fewer than a record for eight steps -- runs of 8 make exactly one for eight, and a block's first
               step and a window's edge start records too, so the runs are twice that)
  short+long   both: the wave-per-path kernel and k_scan, which then takes a full grid
  long, FLATGFA_TAGGED=0   the same item through the directory walk: k_scan's plain untagged build, no emit=two_chunks

For each shape and each kind of call (node depth with unique depth, node depth alone, path_depth_all): k_scan is in the profile
iff the description names it in pass1=; under FLATGFA_SCAN_ALWAYS=1 it always is; the counts are exact (numpy's unique depth,
tests/path_depth_model.py for depth and the paths' sums); the status is clean.  The plans are made with
FLATGFA_DEPTH_PATH=bucketed FLATGFA_BIG_GROUPS=1 FLATGFA_ACC_OWN=0, so that no timed trial decides anything."""
import os
import re

import numpy as np
import pytest

import path_depth_model as pm
from oracle import synth

pytestmark = pytest.mark.gpu

S = 8192
SHAPES = {  # name -> ((paths, steps each, run length) ..., environment)
    "tiny": (((64, 100, 10),), {}),
    "short": (((64, 1000, 10),), {}),
    "long": (((1, 40_000, 16),), {}),
    "short+long": (((64, 1000, 10), (1, 40_000, 16)), {}),
    "long-untagged": (((1, 40_000, 16),), {"FLATGFA_TAGGED": "0"}),
}
KINDS = ("uniq", "depth", "path_depth_all")
PASS1_FOR_ITEMS = {"k_scan", "k_scan_dense", "k_scan_runs"}


def _paths(n_paths, n_steps, run, salt):
    """`n_paths` paths of `n_steps` forward steps in runs of `run` consecutive ids, each run starting at a pseudo-random
    segment (oracle.synth's mix64: the same on every machine)."""
    n_runs = (n_steps + run - 1) // run
    out = np.zeros((n_paths, n_steps), dtype=np.uint32)
    for p in range(n_paths):
        with np.errstate(over="ignore"):
            key = np.uint64(salt + 1 + p) * synth.GOLDEN + np.arange(n_runs, dtype=np.uint64)
        start = (synth.mix64(key) % np.uint64(S - run)).astype(np.int64)
        ids = np.repeat(start, run) + np.tile(np.arange(run), n_runs)
        out[p] = (ids[:n_steps] << 1).astype(np.uint32)
    return out


@pytest.fixture(scope="module")
def shapes():
    """name -> (steps, begin, end, seg_len, the model's answer, unique depth); computed once, never written to."""
    made = {}
    for name, (groups, _) in SHAPES.items():
        if name == "long-untagged":
            made[name] = made["long"]
            continue
        rows = [_paths(n, length, run, 1000 * k).reshape(-1) for k, (n, length, run) in enumerate(groups)]
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for n, length, _ in groups])
        steps = np.concatenate(rows)
        pad = (-len(steps)) % 16  # (the step array ends on a 16-step boundary: every path's last block is in reach)
        steps = np.concatenate([steps, np.zeros(pad, dtype=np.uint32)])
        end = np.cumsum(lens).astype(np.uint32)
        begin = (end - lens).astype(np.uint32)
        seg_len = (1 + np.arange(S, dtype=np.uint32) % 7).astype(np.uint32)
        want = pm.exact(steps, begin, end, seg_len, S)
        uniq = np.zeros(S, dtype=np.int64)
        for b, e in zip(begin, end):
            uniq[np.unique(steps[b:e] >> 1)] += 1
        made[name] = (steps, begin, end, seg_len, want, uniq)
    return made


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("FLATGFA_") and k != "FLATGFA_LIB":
            monkeypatch.delenv(k)
    for k, v in (("FLATGFA_DEPTH_PATH", "bucketed"), ("FLATGFA_BIG_GROUPS", "1"), ("FLATGFA_ACC_OWN", "0")):
        monkeypatch.setenv(k, v)
    return monkeypatch


def _profiled(fn):
    import torch
    from pollen_amd import device as dev
    dev.profile_read()
    dev.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        dev.profile_enable(False)
    return [name for name, _ in dev.profile_read()]


@pytest.mark.parametrize("name", list(SHAPES))
def test_describe_says_what_the_calls_launch(name, shapes, clean_env):
    import torch
    from pollen_amd.device import DepthPlan, DeviceGraph
    steps, begin, end, seg_len, want, want_uniq = shapes[name]
    for k, v in SHAPES[name][1].items():
        clean_env.setenv(k, v)
    plan = DepthPlan(DeviceGraph(steps, begin, end, S, seg_len))
    desc = plan.describe()
    pass1 = re.search(r" pass1=(\S*)", desc).group(1).split("+")
    print(name, "->", desc)
    assert desc.startswith("path=bucketed"), desc
    # the shape is the one the case is about
    lists = {k: int(re.search(rf" {k}_paths=(\d+)", desc).group(1)) for k in ("tiny", "short", "medium")}
    items = int(re.search(r" items=(\d+)", desc).group(1))
    assert (lists["tiny"] > 0) == (name == "tiny") and lists["medium"] == 0, desc
    assert (lists["short"] > 0) == (name in ("short", "short+long")) and (items > 0) == ("long" in name), desc
    assert (" emit=two_chunks" in desc) == (name == "long"), desc
    if name.startswith("long"):  # (the item alone: tagged unless the hook says otherwise)
        assert (" pass2=tagged" in desc) == (name == "long") and (" pass2=directory" in desc) == (name == "long-untagged"), desc
    says_k_scan = bool(PASS1_FOR_ITEMS & set(pass1))
    assert says_k_scan == ("long" in name), desc

    d, u = (torch.full((S,), -1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    ln, wt = (torch.full((len(begin),), -1, dtype=torch.int64, device="cuda:0") for _ in range(2))
    calls = {"uniq": lambda: plan.seg_depth(d, u), "depth": lambda: plan.seg_depth(d), "path_depth_all": lambda: plan.path_depth_all(d, ln, wt)}
    for always in (False, True):
        if always:
            clean_env.setenv("FLATGFA_SCAN_ALWAYS", "1")  # (read by every call)
        for kind in KINDS:
            d.fill_(-1), u.fill_(-1), ln.fill_(-1), wt.fill_(-1)
            names = _profiled(calls[kind])
            plan.status()  # (raises unless clean)
            print(f"  {kind}{' FLATGFA_SCAN_ALWAYS=1' if always else ''}: {' '.join(names)}")
            assert bool(PASS1_FOR_ITEMS & set(names)) == (says_k_scan or always), (kind, always, names, desc)
            for k in ("tiny", "short"):
                assert any(n.startswith(f"k_scan_{k}<") for n in names) == (lists[k] > 0), (kind, names, desc)
            assert (d.cpu().numpy().view(np.uint32) == want.depth).all(), (kind, always)
            if kind == "uniq":
                assert (u.cpu().numpy().view(np.uint32) == want_uniq).all(), (kind, always)
            if kind == "path_depth_all":
                assert ln.cpu().numpy().view(np.uint64).tolist() == want.length, (kind, always)
                assert wt.cpu().numpy().view(np.uint64).tolist() == want.weighted, (kind, always)
    plan.close()
