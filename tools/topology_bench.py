"""validate and degree at scale: one JSON line.

    python tools/topology_bench.py [--out FILE] [--workdir DIR] [--scale N]
    python tools/topology_bench.py --child FILE.flatgfa        (what the kernel trace runs)

The graph is bench.py's cfg-L (synth(1, 1 M segments, 1000 paths of 100 k steps), pangenome model; --scale divides the paths'
length) with the link set its paths induce -- every distinct consecutive step pair, written in one of its two equivalent
forms -- plus the chain i+ -> (i + 1)+, in two states: `valid`, and `dropped` with one link in a thousand removed.  Per state:

  host      flatgfa_validate, host handle to records: the first call (which uploads the links and builds the index, kept
            with the handle) and the best of 3 after it, non-resident (the steps are uploaded per call) and resident
  cpu       tools/topology_cpu.cpp (g++ -O3, one thread: a sorted key vector and a binary search per pair) on the same file,
            best of 3; the records' count and weighted sum and the degrees' must agree with the library's
  kernels   the kernels alone, from `rocprofv3 --kernel-trace --stats` over a child process of its own that makes three
            resident calls (the index kernels run once; the step pass's time is a third of its total), and the step pass
            against its own bytes -- 4 N + 8 P plus the index -- as a fraction of 8 TB/s
"""
import argparse
import csv
import glob
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
import topology_shapes as ts  # noqa: E402
from oracle import flatgfa_oracle as fo  # noqa: E402


def make_graphs(work, scale):
    g = pa.synth(1, 1_000_000, 1000, 100_000 // scale, "pangenome", False)
    p = fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})
    g.close()
    out = {}
    for state, per_million in (("valid", 0), ("dropped", 1000)):
        q = ts.with_links(p, ts.induced_links(p, 0x51, 0xD0, per_million))
        out[state] = os.path.join(work, "cfgL_%s.flatgfa" % state)
        with open(out[state], "wb") as fh:
            fh.write(fo.dump_flatgfa(q))
    return out


def checksums(recs, deg):
    k = np.arange(1, len(recs) + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = recs["path"].astype(np.uint64) + np.uint64(3) * recs["step"] + np.uint64(5) * recs["src"] + np.uint64(7) * recs["dst"]
        h = int((k * v).sum(dtype=np.uint64)) if len(recs) else 0
        hd = int((np.arange(1, len(deg) + 1, dtype=np.uint64) * deg).sum(dtype=np.uint64))
    return "%016x" % h, "%016x" % hd


def best_of(f, n=3):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(min(times), 3)


def child(path):
    g = pa.load(path)
    g.to_device()
    for _ in range(3):
        g.validate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--workdir")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    work = a.workdir or tempfile.mkdtemp(prefix="topology_bench_")
    os.makedirs(work, exist_ok=True)
    files = make_graphs(work, a.scale)
    cpu = os.path.join(work, "topology_cpu")
    subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "topology_cpu.cpp"), "-o", cpu], check=True)
    head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
    res = {"graph": "cfgL with the links its paths induce and the chain", "scale": a.scale, "head": open(head).read().strip() if os.path.exists(head) else "",
           "states": {}}
    for state, path in files.items():
        g = pa.load(path)
        N, P, S, L = len(g.pool("steps")), g.path_count, g.segment_count, len(g.pool("links"))
        r = {"steps": N, "paths": P, "segments": S, "links": L}
        t0 = time.perf_counter()
        recs = g.validate()
        r["host_first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        r["host_ms"] = best_of(g.validate)
        r["degree_ms"] = best_of(g.degree)
        g.to_device()
        g.seg_depth()
        r["resident_ms"] = best_of(g.validate)
        r["records"] = len(recs)
        r["checksum"], r["degree_checksum"] = checksums(recs, g.degree())
        out = json.loads(subprocess.run([cpu, path, "3"], check=True, capture_output=True).stdout)
        for key in ("records", "checksum", "degree_checksum"):
            assert out[key] == r[key], (state, key, out[key], r[key])
        r["cpu_index_ms"], r["cpu_steps_ms"] = out["index_ms"], out["steps_ms"]
        g.close()
        trace = os.path.join(work, "trace_" + state)
        shutil.rmtree(trace, ignore_errors=True)
        pr = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "-o", "t", "--", sys.executable,
                             os.path.abspath(__file__), "--child", path], capture_output=True, timeout=900)
        stats = glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)
        if pr.returncode == 0 and stats:
            rows = [x for x in csv.DictReader(open(stats[0])) if any(k in x["Name"] for k in ("k_steps", "k_link", "k_scan<", "k_spine", "k_sort_rows", "k_long_rows"))]
            r["kernels"] = {x["Name"][:70]: round(float(x["TotalDurationNs"]) / 1e6, 3) for x in rows}
            count = [float(x["TotalDurationNs"]) / 3e6 for x in rows if "k_steps<false>" in x["Name"] or "k_stepsILb0" in x["Name"]]
            if count:
                nbytes = 4 * N + 8 * P + 4 * (2 * S + 1) + 4 * L
                r["step_pass_ms"] = round(count[0], 4)
                r["step_pass_bytes"] = nbytes
                r["step_pass_fraction_of_8TBs"] = round(nbytes / (count[0] * 1e-3) / 8e12, 4)
        else:
            r["kernels"] = None
            r["kernel_trace_error"] = (pr.stderr or b"")[-300:].decode(errors="replace")
        res["states"][state] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if not a.workdir:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
