"""inject at scale: one JSON line.

    python tools/inject_bench.py [--out FILE] [--shapes cfgL,cfgL-4paths] [--lines N] [--chop-before TREE] [--no-chop]
                                 [--goldens] [--slow-odgi] [--host-memory] [--update FILE]

Shapes: cfgL is bench.py's graph (synth(1, 1 M segments, 1000 paths of 100 k steps), pangenome model; segment lengths 1-32);
cfgL-4paths has the same segments under 4 paths of 25 M steps (long paths: the bisections and the big copies).  The BED is
seeded: N = 10^6 intervals on random paths, the start uniform along the path, the length exponential with mean 10 kb.  The
whole result is checked once on the device (every new path is as long in bases as its interval, every old path as long
as it was), then, per shape:

  device       device.inject on the resident image (flatgfa_dev_inject_count + _fill), HIP events, warm, the median of 5: the
               whole call, and the profiled kernels by stage (median per stage); expansion bytes = 4 N read + 4 N' written
               for k_inject_expand_steps + k_inject_copy_lines
  kernels      the kernels alone, from `rocprofv3 --kernel-trace --stats` over a child process of its own that makes three
               device calls on the same graph and lines (no counters): each kernel's total time over the three calls
  host         flatgfa_inject (array entry), host handle to host handle, best of 3, beside what it cannot go below: the
               device call above, a pinned device-to-host copy of its output bytes (4 N' steps + 24 S' segment records + 8 P'
               spans) and a pinned host-to-device copy of the steps it uploads (4 N); the rest is host work (the result's
               pools are allocated and filled, the names appended)
  cpu          tools/inject_cpu.cpp (g++ -O3, one thread: the one-pass model with a sorted key vector) on the same graph and
               BED, the seconds of the work without reading the inputs; its counts and the checksums of its segment lengths
               and path spans must agree with the device's
  chop         tools/chop_bench.py --shapes cfgL --skip-cli in a process of its own in the same session, for the yardstick
               (chop at c = 3 on the same graph); with --chop-before TREE first from that built checkout (the parent
               commit), so that the shared kernels' figure for chop itself is seen before and after

--goldens times FlatGFA.inject (BED text, best of 5) on every fixture of tests/golden/inject/; --slow-odgi times the
reference's `python -m slow_odgi inject --bed` (a process, best of 3) on the same fixtures and needs the reference's slow_odgi
and mygfa on PYTHONPATH and no GPU; --host-memory (with --update) times, for the first shape's output bytes, what the host
route does to the result's pools in host memory whatever the device does: a fresh zero-filled allocation of that size (the
vector's resize) and one copy into it from memory that is already mapped (the staged copy's last hop), best of 3 each, one
thread; --update FILE merges what a run measured into an earlier run's JSON.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pollen_amd as pa  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

STAGES = ["k_inject_positions", "k_inject_locate", "k_inject_cut_table", "k_inject_reduce_segs", "k_inject_reduce_steps",
          "k_inject_reduce_paths", "k_inject_line_spans", "k_inject_reduce_lines", "k_inject_expand_steps", "k_inject_expand_segs",
          "k_inject_copy_lines"]


def make_lines(rng, path_len, n, mean=10_000):
    p = rng.integers(0, len(path_len), n)
    lo = (rng.random(n) * path_len[p]).astype(np.int64)
    hi = np.minimum(lo + rng.exponential(mean, n).astype(np.int64) + 1, path_len[p])
    return p.astype(np.int64), lo, hi


def make_graph(name):
    n_paths, per = {"cfgL": (1000, 100_000), "cfgL-4paths": (4, 25_000_000)}[name]
    g = pa.synth(1, 1_000_000, n_paths, per, "pangenome", False)
    steps, pb, pe, seg_len = g.soa()
    pre = np.concatenate([[0], np.cumsum(seg_len[steps >> 1].astype(np.int64))])
    return g, steps, pb, pe, seg_len, pre[pe] - pre[pb]


def run_shape(name, n_lines, work, cpu_bin):
    import torch
    g, steps, pb, pe, seg_len, path_len = make_graph(name)
    n_paths = len(pb)
    N, S = len(steps), len(seg_len)
    rng = np.random.default_rng(16)
    p, lo, hi = make_lines(rng, path_len, n_lines)
    res = {"shape": name, "n_steps": N, "n_segs": S, "n_paths": n_paths, "n_lines": n_lines}
    dev = torch.device("cuda:0")
    dg = pdev.DeviceGraph(steps, pb, pe, S, seg_len)

    def tensors(k):
        return (torch.from_numpy(p[:k].astype(np.int32)).to(dev), torch.from_numpy(lo[:k]).to(dev), torch.from_numpy(hi[:k]).to(dev))
    # correctness once, on the whole result: every new path is as many bases long as its interval (both ends are on seams
    # now, and the lines lie inside their paths), every old path as long as it was, and no base was lost from a segment
    ids, dlo, dhi = tensors(n_lines)
    out, sf = pdev.inject(dg, ids, dlo, dhi)
    nl = out.seg_len.to(torch.int64)
    c = torch.zeros(out.n_steps + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nl[(out.steps >> 1).to(torch.int64)], 0, out=c[1:])
    got = (c[out.path_end.to(torch.int64)] - c[out.path_begin.to(torch.int64)]).cpu().numpy()
    assert np.array_equal(got[:n_paths], path_len) and np.array_equal(got[n_paths:], hi - lo), name
    assert int(nl.sum()) == int(seg_len.astype(np.int64).sum()) and out.n_paths == n_paths + n_lines, name
    dev_sums = (out.n_steps, out.n_segs, out.n_paths, checksum(out.seg_len.cpu().numpy().view(np.uint32)),
                checksum(np.concatenate([out.path_begin.cpu().numpy().view(np.uint32), out.path_end.cpu().numpy().view(np.uint32)])))
    del out, sf, nl, c, got
    torch.cuda.empty_cache()
    st = torch.cuda.current_stream()

    def dev_once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pdev.profile_read()
        a.record(st)
        o, f = pdev.inject(dg, ids, dlo, dhi)
        b.record(st)
        b.synchronize()
        ks = {}
        for nm, ms in pdev.profile_read():
            if nm.startswith("k_inject"):
                ks[nm] = ks.get(nm, 0.0) + ms
        sizes = (o.n_steps, o.n_segs)
        del o, f
        return a.elapsed_time(b), ks, sizes
    pdev.profile_enable(True)
    dev_once()
    runs = [dev_once() for _ in range(5)]
    pdev.profile_enable(False)
    N2, S2 = runs[0][2]
    res["n_new_steps"], res["n_new_segs"] = N2, S2
    call = [r[0] for r in runs]
    res["device_call_ms_median"] = round(statistics.median(call), 3)
    res["device_call_ms_min_max"] = [round(min(call), 3), round(max(call), 3)]
    stage = {s: round(statistics.median(r[1].get(s, 0.0) for r in runs), 3) for s in STAGES}
    res["stage_ms_median"] = stage
    kern = sum(stage.values())
    res["profiled_kernels_ms"] = round(kern, 3)
    front = stage["k_inject_positions"] + stage["k_inject_locate"] + stage["k_inject_cut_table"]
    res["positions_locate_cut_table_share_of_kernels"] = round(front / kern, 3) if kern else None
    exp_ms = stage["k_inject_expand_steps"] + stage["k_inject_copy_lines"]
    res["expansion_ms"] = round(exp_ms, 3)
    res["expansion_tbps"] = round((4 * N + 4 * N2) / (exp_ms * 1e-3) / 1e12, 3) if exp_ms else None
    del dg, ids, dlo, dhi
    torch.cuda.empty_cache()
    # host handle to host handle (the array entry; the arguments are made outside the clock)
    import ctypes
    from pollen_amd import _lib
    names = [b"n%d" % i for i in range(n_lines)]
    c_names = (ctypes.c_char_p * n_lines)(*names)
    c_lens = (ctypes.c_size_t * n_lines)(*[len(x) for x in names])
    a32, lo64, hi64 = p.astype(np.uint32), lo.astype(np.uint64), hi.astype(np.uint64)

    def host_once():
        h = ctypes.c_void_p()
        t = time.perf_counter()
        rc = _lib.lib().flatgfa_inject(g._h, a32.ctypes.data, lo64.ctypes.data, hi64.ctypes.data, c_names, c_lens, n_lines, 0, ctypes.byref(h))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0, _lib.last_error()
        pa.FlatGFA(h.value).close()
        return ms
    host_once()
    res["flatgfa_inject_ms"] = round(min(host_once() for _ in range(3)), 1)
    out_bytes = 4 * N2 + 24 * S2 + 8 * (n_paths + n_lines)
    dbuf = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    hbuf = torch.empty(out_bytes, dtype=torch.uint8, pin_memory=True)

    def copy_once(dst, src):
        torch.cuda.synchronize()
        t = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    copy_once(hbuf, dbuf)
    res["output_bytes"] = out_bytes
    res["pinned_d2h_ms"] = round(min(copy_once(hbuf, dbuf) for _ in range(3)), 1)
    res["pinned_h2d_steps_ms"] = round(min(copy_once(dbuf[:4 * N], hbuf[:4 * N]) for _ in range(3)), 1)
    res["host_route_rest_ms"] = round(res["flatgfa_inject_ms"] - res["pinned_d2h_ms"] - res["pinned_h2d_steps_ms"] - res["device_call_ms_median"], 1)
    del dbuf, hbuf
    torch.cuda.empty_cache()
    # one CPU thread
    if cpu_bin:
        flat, bed = os.path.join(work, name + ".flatgfa"), os.path.join(work, name + ".bed")
        g.write_flatgfa(flat)
        pn = [g.get_path_name(i) for i in range(n_paths)]
        with open(bed, "wb") as f:
            f.write(b"".join(b"%s\t%d\t%d\tn%d\n" % (pn[int(q)], a, b, i) for i, (q, a, b) in enumerate(zip(p.tolist(), lo.tolist(), hi.tolist()))))
        r = subprocess.run([cpu_bin, flat, bed], check=True, capture_output=True, timeout=3000)
        f = r.stdout.split()
        assert (int(f[0]), int(f[1]), int(f[2]), int(f[4]), int(f[5])) == dev_sums, (name, f, dev_sums)
        res["cpu_1thread_s"] = round(float(f[6]), 3)
        os.unlink(flat)
        os.unlink(bed)
    g.close()
    res["kernel_trace"] = kernel_trace(name, n_lines, work)
    return res


def checksum(a):
    a = np.asarray(a)
    return int(np.bitwise_xor.reduce(a.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.arange(len(a), dtype=np.uint64))) if len(a) else 0


def child(name, n_lines):
    """Three device calls, for the kernel trace."""
    import torch
    g, steps, pb, pe, seg_len, path_len = make_graph(name)
    p, lo, hi = make_lines(np.random.default_rng(16), path_len, n_lines)
    dev = torch.device("cuda:0")
    dg = pdev.DeviceGraph(steps, pb, pe, len(seg_len), seg_len)
    ids, dlo, dhi = torch.from_numpy(p.astype(np.int32)).to(dev), torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    for _ in range(3):
        o, f = pdev.inject(dg, ids, dlo, dhi)
        torch.cuda.synchronize()
        del o, f


def kernel_trace(name, n_lines, work):
    import csv
    import glob
    import shutil
    trace = os.path.join(work, "trace_" + name)
    shutil.rmtree(trace, ignore_errors=True)
    pr = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "-o", "t", "--", sys.executable,
                         os.path.abspath(__file__), "--child", name, "--lines", str(n_lines)], capture_output=True, timeout=900)
    stats = glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)
    if pr.returncode != 0 or not stats:
        return {"error": (pr.stderr or b"")[-300:].decode(errors="replace")}
    rows = sorted(csv.DictReader(open(stats[0])), key=lambda x: -float(x["TotalDurationNs"]))
    return {"calls": 3, "total_ms_over_the_calls": {x["Name"][:90]: round(float(x["TotalDurationNs"]) / 1e6, 3) for x in rows[:16]}}


def goldens(slow):
    import glob
    here = os.path.join(ROOT, "tests", "golden", "inject")
    out = {}
    for bed in sorted(glob.glob(os.path.join(here, "*.inject.bed"))):
        stem = os.path.basename(bed)[:-len(".inject.bed")]
        gfa = os.path.join(here if stem == "synth_inject" else os.path.dirname(here), stem + ".gfa")
        r = {}
        if slow:
            def once():
                t = time.perf_counter()
                subprocess.run([sys.executable, "-m", "slow_odgi", "inject", "--bed", bed, os.path.basename(gfa)], check=True,
                               capture_output=True, cwd=os.path.dirname(gfa), timeout=1200)
                return time.perf_counter() - t
            r["slow_odgi_process_s"] = round(min(once() for _ in range(3)), 3)
        else:
            g = pa.parse(gfa)
            text = open(bed, "rb").read()

            def once():
                t = time.perf_counter()
                q = g.inject(text)
                ms = (time.perf_counter() - t) * 1e3
                q.close()
                return ms
            once()
            r["flatgfa_inject_bed_ms"] = round(min(once() for _ in range(5)), 3)
            r["segments"], r["bed_lines"] = g.segment_count, text.count(b"\n")
            g.close()
        out[stem] = r
    return out


def host_memory(nbytes):
    src = np.ones(nbytes, np.uint8)

    def fill():
        t = time.perf_counter()
        a = np.zeros(nbytes, np.uint8)
        a[::4096] = 0  # (touch every page: calloc alone maps nothing)
        return (time.perf_counter() - t) * 1e3, a
    fills, copies = [], []
    for _ in range(3):
        ms, a = fill()
        fills.append(ms)
        t = time.perf_counter()
        np.copyto(a, src)
        copies.append((time.perf_counter() - t) * 1e3)
        del a
    return {"bytes": nbytes, "fresh_zeroed_allocation_ms": round(min(fills), 1), "copy_into_it_ms": round(min(copies), 1)}


def chop_figure(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "chop_bench.py"), "--shapes", "cfgL", "--skip-cli"], check=True,
                       capture_output=True, timeout=1200)
    d = json.loads(r.stdout.decode().strip().splitlines()[-1])["shapes"][0]
    return {k: d[k] for k in ("device_call_ms", "profiled_kernels_ms", "kernels_tbps", "flatgfa_chop_ms", "n_new_steps")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="cfgL,cfgL-4paths")
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--chop-before")
    ap.add_argument("--no-chop", action="store_true")
    ap.add_argument("--goldens", action="store_true")
    ap.add_argument("--slow-odgi", action="store_true")
    ap.add_argument("--host-memory", action="store_true")
    ap.add_argument("--update")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lines)
    import shutil
    import tempfile
    work = tempfile.mkdtemp(prefix="inject_bench_")
    out = {"bench": "inject"}
    try:
        shapes = [s for s in a.shapes.split(",") if s]
        cpu_bin = None
        if shapes and shutil.which("g++"):
            cpu_bin = os.path.join(work, "inject_cpu")
            subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "inject_cpu.cpp"), "-o", cpu_bin], check=True)
        if shapes:
            out["shapes"] = [run_shape(s, a.lines, work, cpu_bin) for s in shapes]
            if a.chop_before:
                out["chop_c3_cfgL_parent_build"] = chop_figure(a.chop_before)
            if not a.no_chop:
                out["chop_c3_cfgL_this_build"] = chop_figure(ROOT)
        if a.host_memory:
            out["host_memory_of_output"] = host_memory(json.load(open(a.update))["shapes"][0]["output_bytes"])
        if a.goldens:
            out["goldens_flatgfa_inject"] = goldens(False)
        if a.slow_odgi:
            out["goldens_slow_odgi"] = goldens(True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.update:
        old = json.load(open(a.update))
        old.update(out)
        out = old
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
