"""The GFA parser at scale, host and device: one JSON line.

    python tools/parse_bench.py [--segs 1000000] [--paths 1000] [--steps 100000] [--chop 3] [--host-reps 2] [--out FILE]

Two inputs, in one sitting on one box: the text `fgfa print` writes of cfg-L (bench.py's graph: synth(1, 1 M segments,
1000 paths of 100 k steps)) and of cfg-L chopped at 3 (`--chop 0` leaves it out).  Per text:

  host_ms       flatgfa_parse_bytes, the whole call at its defaults: best of --host-reps
  device_ms     flatgfa_parse_bytes_device, the whole call: best of 3 after one warm call
  phases_ms     of the best device call (flatgfa_parse_device_times): the text's upload, every kernel and scan of the
                call by HIP events, of those the two step kernels alone, the pools' download; host_ms there is what is
                left of the call (totals read back, allocations, the name map made on the host)
  floor_ms      a pinned host-to-device copy of the text's bytes plus a pinned device-to-host copy of the pools' bytes
                (torch; the rate of a gigabyte each way, times the bytes): what the whole call is set against
  step_share    the step kernels' rate over the text (bytes / step_ms, both passes read it) as a share of the 6.8 TB/s
                streaming rate of profiles/NOTES.md R6.4

The device route's pools are compared with the host route's, pool for pool, before and after the timed calls; nothing is
reported unless they are equal and the route taken was the device's.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pollen_amd as pa  # noqa: E402

POOLS = ["header", "segs", "paths", "links", "steps", "seq_data", "overlaps", "alignment", "name_data", "optional_data", "line_order"]
STREAM_GBPS = 6800.0  # profiles/NOTES.md R6.4


def same_pools(a, b):
    return all(np.array_equal(a.pool(n), b.pool(n)) for n in POOLS)


def pool_bytes(g):
    return sum(g.pool(n).nbytes for n in POOLS)


def measure(text, host_reps, h2d_gbps, d2h_gbps):
    out = {"text_bytes": len(text)}
    best, host = 1e18, None
    for _ in range(host_reps):
        t = time.perf_counter()
        g = pa.parse_bytes(text)
        best = min(best, time.perf_counter() - t)
        host = host or g
    out["host_ms"] = round(best * 1e3, 1)
    out["segments"], out["paths"], out["steps"] = host.segment_count, host.path_count, len(host.pool("steps"))
    out["pool_bytes"] = pool_bytes(host)
    with pa.parse_bytes_device(text) as g:  # the warm call, checked
        assert g.parsed_on == "device", g.parse_info
        assert same_pools(g, host), "the device route's pools are not the host route's: nothing is reported"
        out["tiles"], out["tile_bytes"] = g.parse_info["tiles"], g.parse_info["tile_bytes"]
    best, phases = 1e18, None
    for _ in range(3):
        t = time.perf_counter()
        g = pa.parse_bytes_device(text)
        dt = time.perf_counter() - t
        if dt < best:
            best, phases = dt, g.parse_info
        last = g
    assert last.parsed_on == "device" and same_pools(last, host), "the device route's pools changed between calls: nothing is reported"
    out["device_ms"] = round(best * 1e3, 1)
    out["phases_ms"] = {k: round(phases[k], 2) for k in ("upload_ms", "kernel_ms", "step_ms", "download_ms")}
    out["phases_ms"]["host_ms"] = round(best * 1e3 - phases["upload_ms"] - phases["kernel_ms"] - phases["download_ms"], 2)
    floor = len(text) / h2d_gbps / 1e6 + out["pool_bytes"] / d2h_gbps / 1e6
    out["floor_ms"] = round(floor, 3)
    out["host_over_device"] = round(out["host_ms"] / (best * 1e3), 2)
    out["device_over_floor"] = round(best * 1e3 / floor, 2)
    step_gbps = 2 * len(text) / phases["step_ms"] / 1e6  # (the count pass and the fill pass each read the text)
    out["step_kernels_gbps"] = round(step_gbps, 1)
    out["step_share_of_streaming_rate"] = round(step_gbps / STREAM_GBPS, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=1_000_000)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--chop", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("parse_bench: no HIP device is visible; nothing is measured without one")
    import torch
    res = {"what": "the GFA parser, host (flatgfa_parse_bytes) and device (flatgfa_parse_bytes_device)",
           "graph": f"synth(1, {args.segs}, {args.paths}, {args.steps}, pangenome)",
           "box": {"cpu": platform.processor() or platform.machine(), "cpus": os.cpu_count(), "gpu": torch.cuda.get_device_name(0),
                   "torch": torch.__version__, "hip": torch.version.hip}}
    head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
    res["box"]["library_head"] = open(head).read() if os.path.exists(head) else None
    n = 1 << 30
    d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    h = torch.zeros(n, dtype=torch.uint8).pin_memory()

    def rate(fn):
        best = 1e18
        for _ in range(4):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        return n / best / 1e9
    res["pinned_h2d_gbps"] = round(rate(lambda: d.copy_(h, non_blocking=True)), 1)
    res["pinned_d2h_gbps"] = round(rate(lambda: h.copy_(d, non_blocking=True)), 1)
    del d, h
    torch.cuda.empty_cache()
    base = pa.synth(1, args.segs, args.paths, args.steps, "pangenome", False)
    inputs = [("cfgL", base)]
    if args.chop:
        inputs.append((f"cfgL_chop{args.chop}", base.chop(args.chop)))
    for key, g in inputs:
        text = g.gfa_text_device()
        g.close()
        res[key] = measure(text, args.host_reps, res["pinned_h2d_gbps"], res["pinned_d2h_gbps"])
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
        del text
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
