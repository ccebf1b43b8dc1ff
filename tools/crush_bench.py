"""Crush at scale: one JSON document (profiles/crush_bench.json).

    python tools/crush_bench.py [--big-bytes 2147483648] [--paths 1000] [--steps 100000] [--out FILE]

Workloads, all on one device in one run:

  cfgL        bench.py's graph with sequences (synth(1, 1 M segments, --paths paths of --steps steps); about 16 MB of bases) with
              1 % of its bases painted over by N runs of mean length 100.  Launch-bound: thirteen launches and one wait for 16 MB.
  big-runs    a device-made pool of --big-bytes bases, segments of 1..63 bases (mean 32) one behind another, 1 % of the bases in
              N runs of 50, 100 or 150
  big-none    the same segments, no N at all: nothing dropped
  big-all     the same segments, every base N: every segment becomes one byte

Per workload: the kernels by stage (HIP events: flatgfa_dev_profile_enable / _read; median, min and max of --reps calls of
device.crush after --warm warm ones), count + fill as bytes read and written per second (the pool once by each, the output
once), a device-to-device copy of the same pool timed in the same run and the ratio of count + fill to it (the floor with
nothing dropped is 1.5: three passes of the memory against the copy's two), the single-thread C++ restatement
(tools/crush_cpu.cpp, g++ -O3 -march=native; its own seconds, memory to memory), and the sha256 of the device's output against
the restatement's before and after the timed calls -- no time is reported unless they are equal.  For cfgL also the whole
flatgfa_crush call, host handle to host handle (best of 3 after a warm one), beside a host-to-device copy of its pool and a
device-to-host copy of its output (torch, pageable memory) and a host copy of the steps it carries over."""
import argparse
import ctypes
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
from pollen_amd import _lib  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

N = 0x4E


def sha(a) -> str:
    return hashlib.sha256(memoryview(np.ascontiguousarray(a))).hexdigest()


def run_cpu(tool, work, seg_seq, pool):
    """The restatement on (u32 spans, u8 pool): (sha256 of its output, kept, dropped, its seconds)."""
    spans, pl, out = (os.path.join(work, n) for n in ("spans.bin", "pool.bin", "out.bin"))
    seg_seq.tofile(spans)
    pool.tofile(pl)
    r = subprocess.run([tool, spans, pl, out], check=True, capture_output=True)
    kept, dropped, _, sec = r.stdout.split()
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for piece in iter(lambda: f.read(1 << 26), b""):
            h.update(piece)
    for p in (spans, pl, out):
        os.unlink(p)
    return h.hexdigest(), int(kept), int(dropped), float(sec)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(name, dg, seg_seq, seq, tool, work, warm, reps):
    import torch
    total = int(seg_seq.cpu().numpy().view(np.uint32)[1::2].astype(np.int64).sum())
    cpu_sha, kept, dropped, cpu_s = run_cpu(tool, work, seg_seq.cpu().numpy().view(np.uint32), seq.cpu().numpy())
    _, out, _ = pdev.crush(dg, seg_seq, seq)
    torch.cuda.synchronize()
    before = sha(out.cpu().numpy())
    del out
    for _ in range(warm):
        pdev.crush(dg, seg_seq, seq)
    torch.cuda.synchronize()
    per = {}
    pdev.profile_enable(True)
    pdev.profile_read()
    for _ in range(reps):
        pdev.crush(dg, seg_seq, seq)
        torch.cuda.synchronize()
        got = {}
        for k, ms in pdev.profile_read():
            got[k] = got.get(k, 0.0) + ms
        for k, ms in got.items():
            per.setdefault(k, []).append(ms)
    pdev.profile_enable(False)
    _, out, _ = pdev.crush(dg, seg_seq, seq)
    torch.cuda.synchronize()
    after = sha(out.cpu().numpy())
    # a device-to-device copy of the same pool, the same way
    dst = torch.empty_like(seq)
    copy = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(seq)
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            copy.append(a.elapsed_time(b))
    res = {"workload": name, "segments": dg.n_segs, "pool_bytes": int(seq.numel()), "laid_out_bytes": total, "kept": kept, "dropped": dropped,
           "sha256_cpu": cpu_sha, "sha256_device_before": before, "sha256_device_after": after, "cpu_restatement_s": cpu_s}
    if not (cpu_sha == before == after) or int(out.numel()) != kept:
        res["error"] = "the device's output is not the restatement's: no time reported"
        return res
    res["kernels_ms"] = {k: stats(v) for k, v in sorted(per.items())}
    cf = [c + f for c, f in zip(per["crush_count"], per["crush_fill"])]
    res["count_plus_fill_ms"] = stats(cf)
    res["bytes_moved"] = 2 * total + kept
    res["count_plus_fill_GBps"] = round((2 * total + kept) / statistics.median(cf) / 1e6, 1)
    res["d2d_copy_ms"] = stats(copy)
    res["d2d_copy_GBps"] = round(2 * int(seq.numel()) / statistics.median(copy) / 1e6, 1)
    res["ratio_to_copy"] = round(statistics.median(cf) / statistics.median(copy), 2)
    res["all_kernels_ms"] = round(sum(statistics.median(v) for v in per.values()), 4)
    return res


def paint_runs(seq, frac, seed):
    """N runs of 50, 100 or 150 bytes over `frac` of seq (a uint8 CUDA tensor), in place."""
    import torch
    n = int(seq.numel())
    g = torch.Generator(device=seq.device)
    g.manual_seed(seed)
    runs = max(1, int(n * frac / 100))
    at = torch.randint(0, max(1, n - 150), (runs,), generator=g, device=seq.device)
    ln = (torch.randint(1, 4, (runs,), generator=g, device=seq.device) * 50)
    for j in range(150):
        seq[at[ln > j] + j] = N


def cfgl(args, tool, work):
    import torch
    g = pa.synth(1, 1_000_000, args.paths, args.steps, "pangenome", True)
    # the runs go into the handle's own pool (a heap handle's memory), so that the handle route crushes what the device pair does
    data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, 5, ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0 and es.value == 1
    pool = np.ctypeslib.as_array(ctypes.cast(data.value, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value,))
    rng = np.random.default_rng(1)
    for at, ln in zip(rng.integers(0, n.value - 150, max(1, n.value // 10000)), rng.integers(1, 4, max(1, n.value // 10000)) * 50):
        pool[at:at + ln] = N
    segs = g.pool("segs")
    seg_seq = np.zeros(2 * len(segs), np.uint32)
    seg_seq[0::2], seg_seq[1::2] = segs["seq_start"], segs["seq_end"] - segs["seq_start"]
    d = torch.device("cuda:0")
    e = torch.zeros(0, dtype=torch.int32, device=d)
    dg = pdev.DeviceGraph.from_tensors(e, e, e, len(segs), torch.from_numpy((seg_seq[1::2]).view(np.int32).copy()).to(d))
    t_seg, t_seq = torch.from_numpy(seg_seq.view(np.int32)).to(d), torch.from_numpy(pool.copy()).to(d)
    res = measure("cfgL", dg, t_seg, t_seq, tool, work, args.warm, args.reps)
    res["note"] = "launch-bound: the check, the count, three scans, the lengths and the fill are thirteen launches and one wait around 16 MB"
    # the whole call, host handle to host handle
    q = g.crush()
    res["handle_sha256"] = sha(q.pool("seq_data"))
    walls = []
    for _ in range(3):
        q.close()
        t0 = time.perf_counter()
        q = g.crush()
        walls.append((time.perf_counter() - t0) * 1e3)
    res["flatgfa_crush_ms"] = stats(walls)
    out = q.pool("seq_data")
    q.close()
    t0 = time.perf_counter()
    up = torch.from_numpy(pool).to(d)
    up2 = torch.from_numpy(seg_seq.view(np.int32)).to(d)
    torch.cuda.synchronize()
    res["h2d_pool_and_spans_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    dev_out = torch.from_numpy(out).to(d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev_out.cpu()
    res["d2h_output_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    steps = g.pool("steps")
    t0 = time.perf_counter()
    steps.copy()
    res["host_copy_of_steps_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["steps"] = int(len(steps))
    del up, up2
    g.close()
    return res


def big(args, tool, work):
    import torch
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(7)
    n_segs = args.big_bytes // 32
    lens = torch.randint(1, 64, (n_segs,), generator=g, device=d, dtype=torch.int64)
    end = torch.cumsum(lens, 0)
    total = int(end[-1])
    assert total < (1 << 32)
    seg_seq = torch.stack([end - lens, lens], dim=1).to(torch.int32).reshape(-1).contiguous()  # (u32 bits)
    e = torch.zeros(0, dtype=torch.int32, device=d)
    dg = pdev.DeviceGraph.from_tensors(e, e, e, n_segs, lens.to(torch.int32))
    del lens, end
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=d)
    out = []
    for name in ("big-runs", "big-none", "big-all"):
        if name == "big-all":
            seq = torch.full((total,), N, dtype=torch.uint8, device=d)
        else:
            seq = letters[torch.randint(0, 4, (total,), generator=g, device=d)]
            if name == "big-runs":
                paint_runs(seq, 0.01, 11)
        out.append(measure(name, dg, seg_seq, seq, tool, work, args.warm, args.reps))
        del seq
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-bytes", type=int, default=1 << 31)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with tempfile.TemporaryDirectory() as work:
        tool = os.path.join(work, "crush_cpu")
        subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", os.path.join(ROOT, "tools", "crush_cpu.cpp"), "-o", tool])
        head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
        res = {"what": "crush (fgfa crush)", "device": torch.cuda.get_device_name(0), "build": open(head).read() if os.path.exists(head) else "unknown",
               "warm": args.warm, "reps": args.reps, "workloads": [cfgl(args, tool, work)] + big(args, tool, work)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
