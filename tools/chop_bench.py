"""chop at scale: one JSON line.

    python tools/chop_bench.py [--out FILE] [--shapes cfgL,cfgL-chrom,giant] [--workdir DIR] [--skip-cli]

Shapes: cfgL and cfgL-chrom are bench.py's graphs (synth(1, 1 M segments, 1000 paths of 100 k steps), pangenome and chromosome
models; segment lengths 1-32) at c = 3; giant is 200 000 segments of 1-4 bp and four of 2-5 Mbp, 16 paths of 1 M steps that
step the giants 12 times in all, both orientations, at c = 1.  Each shape's result is checked against the numpy model
(tests/chop_model.py) once, on the steps' checksum and the totals.  Then, per shape:

  kernels      device.chop on the resident image (flatgfa_dev_chop_count + _fill), HIP events, best of 5: the whole call, and
               the sum of the profiled kernels; bytes = 4 N read + 4 N' written, against 8 TB/s
  host         FlatGFA.chop, host handle to host handle, best of 3, beside a pinned device-to-host copy of its output bytes
               (4 N' steps + 24 S' segment records)
  cli          `fgfa -i G.flatgfa -o OUT.flatgfa chop -c C`, whole process, and tools/chop_cpu.cpp (g++ -O3, one thread) on the
               same file: their step checksums must agree
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pollen_amd as pa  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402
from oracle import flatgfa_oracle as fo  # noqa: E402

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
PEAK = 8e12


def giant_pools():
    rng = np.random.default_rng(9)
    S = 200_004
    lens = rng.integers(1, 5, S).astype(np.int64)
    giants = np.array([7, 70_000, 140_000, 200_000])
    lens[giants] = [5_000_000, 3_000_001, 2_000_003, 4_321_987]
    st = np.concatenate([[0], np.cumsum(lens)[:-1]])
    segs = np.zeros(S, fo.SEG_DT)
    segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, S + 1), st, st + lens
    P, L = 16, 1_000_000
    s = rng.integers(0, S, P * L).astype(np.uint32)
    s[s == giants[0]] = 0
    s[s == giants[1]] = 1
    s[s == giants[2]] = 2
    s[s == giants[3]] = 3
    s[rng.choice(P * L, 12, replace=False)] = np.tile(giants, 3)
    steps = (s << 1) | rng.integers(0, 2, P * L).astype(np.uint32)
    names = b"".join(b"p%02d" % k for k in range(P))
    paths = np.zeros(P, fo.PATH_DT)
    paths["name_start"], paths["name_end"] = np.arange(P) * 3, np.arange(P) * 3 + 3
    paths["steps_start"], paths["steps_end"] = np.arange(P) * L, np.arange(P) * L + L
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=paths, links=np.zeros(0, fo.LINK_DT), steps=steps,
                    seq_data=np.full(int(lens.sum()), ord("A"), np.uint8), overlaps=np.zeros(0, fo.SPAN_DT),
                    alignment=np.zeros(0, np.uint32), name_data=np.frombuffer(names, np.uint8).copy(), optional_data=z, line_order=z)


def make_shape(name, workdir):
    path = os.path.join(workdir, name + ".flatgfa")
    if name == "giant":
        with open(path, "wb") as f:
            f.write(fo.dump_flatgfa(giant_pools()))
        return path, 1
    model = {"cfgL": "pangenome", "cfgL-chrom": "chromosome"}[name]
    pa.synth(1, 1_000_000, 1000, 100_000, model, False).write_flatgfa(path)
    return path, 3


def best(fn, reps):
    out = []
    for _ in range(reps):
        out.append(fn())
    return min(out)


def checksum(steps):
    return int(np.bitwise_xor.reduce(steps.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.arange(len(steps), dtype=np.uint64))) if len(steps) else 0


def run_shape(name, workdir, skip_cli, cpu_bin):
    import torch
    import chop_model as cm
    path, c = make_shape(name, workdir)
    g = pa.load(path)
    steps, pb, pe, seg_len = g.soa()
    N, S = len(steps), len(seg_len)
    res = {"shape": name, "c": c, "n_steps": N, "n_segs": S}
    # correctness once, against the numpy model (totals and the steps' checksum)
    want = cm.chop_fast(cm.pools_of(g), c)
    res["n_new_steps"], res["n_new_segs"] = len(want.steps), len(want.segs)
    want_sum = checksum(want.steps)
    del want
    dg = pdev.DeviceGraph(steps, pb, pe, S, seg_len)
    out, sf = pdev.chop(dg, c)
    got = out.steps.cpu().numpy().view(np.uint32)
    assert checksum(got) == want_sum and out.n_segs == res["n_new_segs"], name
    del out, sf, got
    N2, S2 = res["n_new_steps"], res["n_new_segs"]
    # (a) kernels on the resident image
    st = torch.cuda.current_stream()

    def dev_once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pdev.profile_read()
        a.record(st)
        o, f = pdev.chop(dg, c)
        b.record(st)
        b.synchronize()
        ks = sum(ms for nm, ms in pdev.profile_read() if nm.startswith("k_chop"))
        del o, f
        return a.elapsed_time(b), ks
    pdev.profile_enable(True)
    dev_once()
    runs = [dev_once() for _ in range(5)]
    pdev.profile_enable(False)
    call_ms = min(r[0] for r in runs)
    kern_ms = min(r[1] for r in runs)
    nbytes = 4 * N + 4 * N2
    res["device_call_ms"] = round(call_ms, 3)
    res["profiled_kernels_ms"] = round(kern_ms, 3)
    res["device_call_tbps"] = round(nbytes / (call_ms * 1e-3) / 1e12, 3)
    res["device_call_pct_of_8tbps"] = round(100 * nbytes / (call_ms * 1e-3) / PEAK, 1)
    res["kernels_tbps"] = round(nbytes / (kern_ms * 1e-3) / 1e12, 3) if kern_ms else None
    del dg
    torch.cuda.empty_cache()
    # (b) host to host, beside a pinned copy of the output bytes
    def host_once():
        t = time.perf_counter()
        q = g.chop(c)
        ms = (time.perf_counter() - t) * 1e3
        q.close()
        return ms
    host_once()
    res["flatgfa_chop_ms"] = round(best(host_once, 3), 1)
    out_bytes = 4 * N2 + 24 * S2
    dbuf = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    hbuf = torch.empty(out_bytes, dtype=torch.uint8, pin_memory=True)

    def copy_once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        hbuf.copy_(dbuf, non_blocking=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    copy_once()
    res["pinned_d2h_ms"] = round(best(copy_once, 3), 1)
    res["flatgfa_chop_over_pinned_copy"] = round(res["flatgfa_chop_ms"] / res["pinned_d2h_ms"], 2)
    del dbuf, hbuf
    g.close()
    # (c) the process, and one CPU thread
    if not skip_cli:
        outp = os.path.join(workdir, name + ".chop.flatgfa")
        t = time.perf_counter()
        subprocess.run([FGFA, "-i", path, "-o", outp, "chop", "-c", str(c)], check=True, timeout=1200)
        res["cli_s"] = round(time.perf_counter() - t, 3)
        q = pa.load(outp)
        assert checksum(q.pool("steps")) == want_sum
        q.close()
        os.unlink(outp)
        if cpu_bin:
            t = time.perf_counter()
            r = subprocess.run([cpu_bin, path, str(c)], check=True, capture_output=True, timeout=3600)
            res["cpu_1thread_s"] = round(time.perf_counter() - t, 3)
            assert int(r.stdout.split()[0]) == N2, r.stdout
    os.unlink(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="cfgL,cfgL-chrom,giant")
    ap.add_argument("--workdir")
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="chop_bench_")
    cpu_bin = None
    if not a.skip_cli and shutil.which("g++"):
        cpu_bin = os.path.join(work, "chop_cpu")
        subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "chop_cpu.cpp"), "-o", cpu_bin], check=True)
    try:
        out = {"bench": "chop", "shapes": [run_shape(s, work, a.skip_cli, cpu_bin) for s in a.shapes.split(",")]}
    finally:
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
