"""Flatten where the offsets pass 2^32: three segments of 2^31 bases and one of 5.  No host handle can hold the six gigabytes
of sequence behind them, and the BED reads none, so tests/device_check/flatten_check.hip calls flatten_device.hpp directly
(`make -C pollen_amd/csrc flatten_check`); flatgfa_dev_flatten_legend gets the same lengths through ctypes.  Run with -m gpu."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chop_shapes as cs
import flatten_model as fm
import pollen_amd as pa  # noqa: F401
from conftest import ROOT
from pollen_amd import _lib

pytestmark = pytest.mark.gpu
CHECK = os.path.join(ROOT, "pollen_amd", "build", "flatten_check")
LENS = [2**31, 2**31, 2**31, 5]
PATHS = [(b"left", [0, 3, 5, 6, 7]), (b"a_longer_name", [6, 4, 2, 1])]
NAME = b"big.og"


def model():
    """The same graph as Pools (the lengths as spans from 0: the model reads the spans and no base)."""
    steps = [h for _, hs in PATHS for h in hs]
    spans, at = [], 0
    for _, hs in PATHS:
        spans.append((at, at + len(hs)))
        at += len(hs)
    p = cs.make_pools(LENS, steps, spans, seq=False)
    names = b"".join(n for n, _ in PATHS)
    p.name_data = np.frombuffer(names, np.uint8).copy()
    ends = np.cumsum([len(n) for n, _ in PATHS])
    p.paths["name_start"], p.paths["name_end"] = ends - [len(n) for n, _ in PATHS], ends
    return p


def build():
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "pollen_amd", "csrc"), "flatten_check"], check=True, capture_output=True, timeout=600)


@pytest.mark.parametrize("chunk", [None, 2])
def test_offsets_past_2_32(tmp_path, chunk):
    build()
    p = model()
    leg = fm.legend(p)
    assert leg == [0, 2**31, 2**32, 3 * 2**31, 3 * 2**31 + 5]
    (tmp_path / "in.txt").write_bytes(NAME + b"\n" + b" ".join(b"%d" % x for x in LENS) + b"\n" +
                                      b"".join(n + b" " + b" ".join(b"%d" % h for h in hs) + b"\n" for n, hs in PATHS))
    args = [CHECK, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")] + ([str(chunk)] if chunk else [])
    r = subprocess.run(["timeout", "-k", "10", "60", *args], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "out.txt").read_bytes()
    want = b"legend " + b" ".join(b"%d" % x for x in leg) + b"\n" + fm.bed(p, NAME)
    assert got == want
    assert b"\t6442450944\t6442450949\t" in got  # a start and an end past 2^32


def test_dev_legend_past_2_32():
    import torch
    d = torch.device("cuda:0")
    seg_len = torch.tensor(LENS, dtype=torch.int64).to(torch.int32).to(d)  # (u32 bits)
    out = torch.full((len(LENS) + 1 + 8,), -1, dtype=torch.int64, device=d)
    g = _lib.flatgfa_dev_graph_t(None, 0, None, None, 0, len(LENS), seg_len.data_ptr())
    torch.cuda.synchronize()
    assert _lib.lib().flatgfa_dev_flatten_legend(ctypes.byref(g), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:5].tolist() == [0, 2**31, 2**32, 3 * 2**31, 3 * 2**31 + 5] and (got[5:] == -1).all()
    # no lengths: an argument error, and no segments: the one zero
    g0 = _lib.flatgfa_dev_graph_t(None, 0, None, None, 0, len(LENS), None)
    assert _lib.lib().flatgfa_dev_flatten_legend(ctypes.byref(g0), out.data_ptr(), None) == -1
    g1 = _lib.flatgfa_dev_graph_t(None, 0, None, None, 0, 0, seg_len.data_ptr())
    assert _lib.lib().flatgfa_dev_flatten_legend(ctypes.byref(g1), out.data_ptr() + 8, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:3].tolist() == [0, 0, 2**32]
