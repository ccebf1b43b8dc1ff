"""extract at scale: one JSON line.

    python tools/extract_bench.py [--out FILE] [--workdir DIR] [--dists 1,4,16] [--skip-literal-above N]
    python tools/extract_bench.py --child FILE.flatgfa ORIGIN DIST        (what the kernel trace runs)

The graph is bench.py's cfg-L (synth(1, 1 M segments, 1000 paths of 100 k steps), pangenome model) with sequences, and with
links: the chain i -> i + 1 and 100 000 random ones, random orientations, a third of them with a one-op alignment.  For each
-c, at the defaults (-d 300000 -e 6), from the segment in the middle:

  host      flatgfa_extract, host handle to host handle: the first call (which also puts the sequence pool on the device, kept
            with the handle) and the best of 3 after it
  cpu       tools/extract_cpu.cpp (g++ -O3, one thread) on the same file, best of 3, in both forms -- `literal` (every frontier
            segment reads all links, as extract.rs does) and `levelwise` (one link pass per level) -- so that a speed-up is
            not credited to the reference's quadratic walk.  Sizes and a weighted sum of the pools must agree with the library's.
  kernels   the kernels alone, from `rocprofv3 --kernel-trace --stats` over a child process of its own that makes three calls
            (the sum of all kernel time divided by 3)
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
from oracle import flatgfa_oracle as fo  # noqa: E402


def extract_id(g, origin, c, d=300000, e=6):
    import ctypes
    from pollen_amd import _lib
    h = ctypes.c_void_p()
    rc = _lib.lib().flatgfa_extract(g._h, origin, c, d, e, ctypes.byref(h))
    if rc:
        raise pa.FlatGFAError("extract", rc)
    return pa.FlatGFA(h.value)


def make_graph(path):
    g = pa.synth(1, 1_000_000, 1000, 100_000, "pangenome", True)
    p = fo.Pools(**{n: g.pool(n) for n in fo.POOL_ORDER})
    g.close()
    rng = np.random.default_rng(11)
    S = len(p.segs)
    f = np.concatenate([np.arange(S - 1), rng.integers(0, S, 100_000)]).astype(np.uint32)
    t = np.concatenate([np.arange(1, S), rng.integers(0, S, 100_000)]).astype(np.uint32)
    lk = np.zeros(len(f), fo.LINK_DT)
    lk["from_"] = (f << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    lk["to"] = (t << 1) | rng.integers(0, 2, len(f)).astype(np.uint32)
    n_ops = (rng.random(len(f)) < 1 / 3).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n_ops)])
    lk["ov_start"], lk["ov_end"] = off[:-1], off[1:]
    p.links = lk
    p.alignment = (rng.integers(1, 50, int(off[-1])) << 8).astype(np.uint32)
    with open(path, "wb") as fh:
        fh.write(fo.dump_flatgfa(p))
    return S


def wsum(a):
    a = np.ascontiguousarray(a).astype(np.uint64)
    return int((a * np.arange(1, len(a) + 1, dtype=np.uint64)).sum(dtype=np.uint64)) if len(a) else 0


def sizes(q):
    links = q.pool("links")
    h = (wsum(q.pool("steps")) + wsum(q.pool("segs")["name"]) + wsum(q.pool("name_data")) + wsum(q.pool("seq_data")) +
         wsum(links.view(np.uint32))) % (1 << 64)
    return {"segs": q.segment_count, "paths": q.path_count, "links": len(links), "steps": len(q.pool("steps")),
            "seq_bytes": len(q.pool("seq_data")), "checksum": "%016x" % h}


def child(path, origin, dist):
    g = pa.load(path)
    for _ in range(3):
        extract_id(g, origin, dist).close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--workdir")
    ap.add_argument("--dists", default="1,4,16")
    ap.add_argument("--skip-literal-above", type=float, default=3e10, help="frontier segments x links beyond which the literal form is not run")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]))
    work = a.workdir or tempfile.mkdtemp(prefix="extract_bench_")
    os.makedirs(work, exist_ok=True)
    path = os.path.join(work, "cfgL_links.flatgfa")
    S = make_graph(path)
    cpu = os.path.join(work, "extract_cpu")
    subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "extract_cpu.cpp"), "-o", cpu], check=True)
    origin = S // 2
    g = pa.load(path)
    n_links = len(g.pool("links"))
    res = {"graph": "cfgL with sequences and links", "segments": S, "steps": 100_000_000, "links": n_links, "origin": origin, "d": 300000, "e": 6,
           "head": open(os.path.join(ROOT, "pollen_amd", "lib", "HEAD")).read().strip() if os.path.exists(os.path.join(ROOT, "pollen_amd", "lib", "HEAD")) else "",
           "dists": {}}
    for k, c in enumerate(int(x) for x in a.dists.split(",")):
        r = {}
        t0 = time.perf_counter()
        q = extract_id(g, origin, c)
        first = (time.perf_counter() - t0) * 1e3
        if k == 0:
            r["host_first_call_ms"] = round(first, 3)  # (with the upload of the sequence pool)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            extract_id(g, origin, c).close()
            times.append((time.perf_counter() - t0) * 1e3)
        r["host_ms"] = round(min(times), 3)
        r["result"] = sizes(q)
        for form in ("levelwise", "literal"):
            if form == "literal" and r["result"]["segs"] * n_links > a.skip_literal_above:
                r["cpu_literal"] = "not run: %d segments x %d links" % (r["result"]["segs"], n_links)
                continue
            out = json.loads(subprocess.run([cpu, path, str(origin), str(c), "300000", "6", form, "3"], check=True, capture_output=True).stdout)
            for key in ("segs", "paths", "links", "steps", "seq_bytes", "checksum"):
                assert out[key] == r["result"][key], (form, key, out[key], r["result"][key])
            r["cpu_%s_ms" % form] = out["ms"]
        trace = os.path.join(work, "trace_c%d" % c)
        shutil.rmtree(trace, ignore_errors=True)
        pr = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "-o", "t", "--", sys.executable,
                             os.path.abspath(__file__), "--child", path, str(origin), str(c)], capture_output=True, timeout=900)
        files = glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)
        if pr.returncode == 0 and files:
            rows = list(csv.DictReader(open(files[0])))
            r["kernels_ms"] = round(sum(float(x["TotalDurationNs"]) for x in rows) / 3e6, 3)
            r["kernels"] = {x["Name"][:60]: round(float(x["TotalDurationNs"]) / 3e6, 3) for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:6]}
        else:
            r["kernels_ms"] = None
            r["kernel_trace_error"] = (pr.stderr or b"")[-300:].decode(errors="replace")
        res["dists"][str(c)] = r
        q.close()
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
