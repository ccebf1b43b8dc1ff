"""Flip at scale: one JSON document (profiles/flip_bench.json).

    python tools/flip_bench.py [--paths 1000] [--steps 100000] [--links 100000] [--out FILE]

Workloads, both bench.py's graphs with sequences, on one device in one run:

  cfgL         synth(1, 1 M segments, --paths paths of --steps steps, pangenome): one step in twenty walks backward, so no path
               turns -- the weighing, and a key table of the old links alone
  cfgL-chrom   the same sizes, chromosome model: every other path runs down the graph, so half the paths turn and every step
               of theirs but the last brings a candidate link

The synthetic graphs have no links; the device-level workloads get --links old ones, the consecutive step pairs of path 0 with
the overlap 0M (the handle route runs on the graph as it is).  Per workload: device.flip on the resident image (wall clock
around the call and a synchronize: median, min and max of --reps calls after --warm warm ones), the kernel groups by HIP
events (flatgfa_dev_profile_enable / _read: flip_weigh -- weigh, decide, the two scans over the paths; flip_group -- keys,
rows, sort and decide; flip_compact_count and flip_compact -- the keep flags' scans and the stores; flip_rewrite), a
device-to-device copy of the step array and a pinned host-to-device copy of the pools the call reads, timed in the same run,
the whole flatgfa_flip call, host handle to host handle (best of 3 after a warm one), and the single-thread C++ restatement
(tools/flip_cpu.cpp, g++ -O3 -march=native; its own seconds, memory to memory).  The sha256 of the device's steps, flags and
links is held against the restatement's before and after the timed calls -- no time is reported unless they are equal."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pollen_amd as pa  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

FILES = ("steps.bin", "spans.bin", "seglen.bin", "links.bin", "align.bin", "out_steps.bin", "out_turned.bin", "out_links.bin")


def sha(a) -> str:
    return hashlib.sha256(memoryview(np.ascontiguousarray(a))).hexdigest()


def sha_file(path) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 26), b""):
            h.update(piece)
    return h.hexdigest()


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_cpu(tool, work, arrays):
    paths = [os.path.join(work, n) for n in FILES]
    for a, path in zip(arrays, paths):
        np.ascontiguousarray(a).tofile(path)
    r = subprocess.run([tool] + paths, check=True, capture_output=True)
    turned, kept, new, sec = r.stdout.split()
    shas = [sha_file(p) for p in paths[5:]]
    for p in paths:
        os.unlink(p)
    return shas, int(turned), int(kept), int(new), float(sec)


def device_shas(out):
    new, links_out, turned = out
    return [sha(new.steps.cpu().numpy()), sha(turned.cpu().numpy().astype(np.uint8)), sha(links_out.cpu().numpy())]


def workload(name, model, args, tool, work):
    import torch
    d = torch.device("cuda:0")
    g = pa.synth(1, 1_000_000, args.paths, args.steps, model, True)
    steps, paths, segs = g.pool("steps"), g.pool("paths"), g.pool("segs")
    seg_len = (segs["seq_end"] - segs["seq_start"]).astype(np.uint32)
    spans = np.zeros(2 * len(paths), np.uint32)
    spans[0::2], spans[1::2] = paths["steps_start"], paths["steps_end"]
    first = steps[int(spans[0]):int(spans[1])][:args.links + 1]
    links = np.zeros((max(len(first) - 1, 0), 4), np.uint32)
    links[:, 0], links[:, 1], links[:, 3] = first[:-1], first[1:], 1
    align = np.zeros(1, np.uint32)
    cpu_shas, n_turned, kept, new, cpu_s = run_cpu(tool, work, (steps, spans, seg_len, links, align))
    dg = pdev.DeviceGraph(steps, spans[0::2], spans[1::2], len(segs), seg_len)
    t_links = torch.from_numpy(links.view(np.int32).reshape(-1).copy()).to(d)
    t_align = torch.from_numpy(align.view(np.int32).copy()).to(d)
    call = lambda: pdev.flip(dg, t_links, alignment=t_align)  # noqa: E731
    before = device_shas(call())
    for _ in range(args.warm):
        call()
    torch.cuda.synchronize()
    walls, per = [], {}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del out
    pdev.profile_enable(True)
    pdev.profile_read()
    for _ in range(args.reps):
        call()
        torch.cuda.synchronize()
        got = {}
        for k, ms in pdev.profile_read():
            got[k] = got.get(k, 0.0) + ms
        for k, ms in got.items():
            per.setdefault(k, []).append(ms)
    pdev.profile_enable(False)
    after = device_shas(call())
    res = {"workload": name, "model": model, "segments": len(segs), "paths": len(paths), "steps": int(len(steps)), "links_in": int(len(links)),
           "turned": n_turned, "links_out": kept, "links_new": new, "sha256_cpu": cpu_shas, "sha256_device_before": before, "sha256_device_after": after,
           "cpu_restatement_s": cpu_s}
    if not (cpu_shas == before == after):
        res["error"] = "the device's output is not the restatement's: no time reported"
        g.close()
        return res
    res["device_flip_wall_ms"] = stats(walls)
    res["kernels_ms"] = {k: stats(v) for k, v in sorted(per.items())}
    res["all_kernels_ms"] = round(sum(statistics.median(v) for v in per.values()), 4)
    # the yardsticks, the same way: a device-to-device copy of the steps, and a pinned copy of what the call reads
    dst = torch.empty_like(dg.steps)
    pinned = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).pin_memory() for a in (steps, spans, seg_len, links)]
    room = [torch.empty_like(t, device=d) for t in pinned]
    copy, h2d = [], []
    for i in range(args.warm + args.reps):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        dst.copy_(dg.steps)
        b.record()
        for src, to in zip(pinned, room):
            to.copy_(src, non_blocking=True)
        c.record()
        torch.cuda.synchronize()
        if i >= args.warm:
            copy.append(a.elapsed_time(b))
            h2d.append(b.elapsed_time(c))
    res["d2d_copy_of_steps_ms"] = stats(copy)
    res["pinned_h2d_of_pools_ms"] = stats(h2d)
    res["pools_bytes"] = int(sum(t.numel() * 4 for t in pinned))
    wr = statistics.median(per["flip_weigh"]) + statistics.median(per["flip_rewrite"])
    res["weigh_plus_rewrite_ms"] = round(wr, 4)
    res["weigh_plus_rewrite_to_copy"] = round(wr / statistics.median(copy), 2)  # (the floor is 1.5: the steps are read twice and written once)
    res["all_kernels_to_copy"] = round(res["all_kernels_ms"] / statistics.median(copy), 2)
    res["restatement_to_device_wall"] = round(cpu_s * 1e3 / statistics.median(walls), 1)
    # the whole call, host handle to host handle (the graph as it is: no links)
    q = g.flip()
    res["handle_turned_and_links"] = list(g.flip_count())
    res["handle_steps_sha256_is_the_devices"] = sha(q.pool("steps")) == before[0]
    hw = []
    for _ in range(3):
        q.close()
        t0 = time.perf_counter()
        q = g.flip()
        hw.append((time.perf_counter() - t0) * 1e3)
    q.close()
    res["flatgfa_flip_ms"] = stats(hw)
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--links", type=int, default=100_000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with tempfile.TemporaryDirectory() as work:
        tool = os.path.join(work, "flip_cpu")
        subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", os.path.join(ROOT, "tools", "flip_cpu.cpp"), "-o", tool])
        head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
        res = {"what": "flip (fgfa flip)", "device": torch.cuda.get_device_name(0), "build": open(head).read() if os.path.exists(head) else "unknown",
               "warm": args.warm, "reps": args.reps,
               "workloads": [workload("cfgL", "pangenome", args, tool, work), workload("cfgL-chrom", "chromosome", args, tool, work)]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
