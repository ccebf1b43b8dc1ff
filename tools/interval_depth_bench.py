"""Window depth over every path at scale: one JSON line.

    python tools/interval_depth_bench.py [--out FILE] [--scale N] [--window W] [--runs R]

The graph is bench.py's cfg-L (synth(1, 1 M segments, 1000 paths of 100 k steps), pangenome model; --scale divides the paths'
length), the workload windows of W = 1000 bases along every path, on one resident handle:

  per_path    the route there was before: flatgfa_window_depth_table once per path (each call fetches the depth vector and
              walks its path on the host), the tables concatenated
  all_paths   flatgfa_window_depth_paths_table: one call, the interval walk on the device; the whole call, and the kernels by
              their HIP events (flatgfa_dev_profile_read: the interval job's three stages, and the depth pass before them)
  cuts        the interval kernels' event time with the lane / wave cut as it ships and one alternative either side of it

The two routes' bytes are compared before either is timed; a difference ends the run.  Every time is the median of R runs
(after one that is not timed), with the least and the most.  There is no fallback: without a device the first call fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pollen_amd as pa  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

CUT_HOOK = "FLATGFA_INTERVAL_LANE_CUT"
SHIPPED_CUT = 8  # kIntervalLaneCut of pollen_amd/csrc/interval_device.hpp
CUTS = (2, SHIPPED_CUT, 32)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def timed(f, runs):
    f()  # (not timed)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def kernel_times(g, window, runs):
    """{stage: spread} of the profiled stages of `runs` calls, and the whole calls' spread with the profiler on."""
    per_stage, whole = {}, []
    g.window_depth_paths_table(window)
    for _ in range(runs):
        pdev.profile_enable(True)
        pdev.profile_read()
        try:
            t0 = time.perf_counter()
            g.window_depth_paths_table(window)
            whole.append((time.perf_counter() - t0) * 1e3)
        finally:
            pdev.profile_enable(False)
        sums = {}
        for name, ms in pdev.profile_read():
            key = name if name.startswith("interval_") else "depth_pass"
            sums[key] = sums.get(key, 0.0) + ms
        sums["interval_all"] = sum(v for k, v in sums.items() if k.startswith("interval_"))
        for k, v in sums.items():
            per_stage.setdefault(k, []).append(v)
    return {k: spread(v) for k, v in per_stage.items()}, spread(whole)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--per-path-runs", type=int, default=3)
    a = ap.parse_args()
    os.environ.pop(CUT_HOOK, None)
    g = pa.synth(1, 1_000_000, 1000, 100_000 // a.scale, "pangenome", False)
    P = g.path_count
    g.to_device()
    g.seg_depth()

    def per_path():
        return b"".join(g.window_depth_table(i, a.window) for i in range(P))

    def all_paths():
        return g.window_depth_paths_table(a.window)

    old, new = per_path(), all_paths()
    if old != new:
        raise SystemExit("the two routes' tables differ: %d and %d bytes" % (len(old), len(new)))
    head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
    res = {"graph": "cfgL", "scale": a.scale, "head": open(head).read().strip() if os.path.exists(head) else "", "steps": len(g.pool("steps")),
           "paths": P, "segments": g.segment_count, "window": a.window, "windows": new.count(b"\n"), "table_bytes": len(new),
           "tables_equal": True, "lane_cut": SHIPPED_CUT}
    res["per_path"] = timed(per_path, a.per_path_runs)
    res["all_paths"] = {"call": timed(all_paths, a.runs)}
    res["all_paths"]["kernels"], res["all_paths"]["call_profiled"] = kernel_times(g, a.window, a.runs)
    res["cuts"] = {}
    for cut in CUTS:
        os.environ[CUT_HOOK] = str(cut)
        try:
            if all_paths() != new:
                raise SystemExit("cut %d changes the table" % cut)
            k, _ = kernel_times(g, a.window, a.runs)
            res["cuts"][str(cut)] = {"interval_depth": k.get("interval_depth"), "interval_all": k.get("interval_all")}
        finally:
            os.environ.pop(CUT_HOOK, None)
    res["speedup_call_over_per_path"] = round(res["per_path"]["median_ms"] / res["all_paths"]["call"]["median_ms"], 2)
    g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
