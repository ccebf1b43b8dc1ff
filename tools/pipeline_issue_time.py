#!/usr/bin/env python3
"""The host's share of a pipelined depth call (flatgfa_dev_pipeline_seg_depth): how long the host takes to enqueue calls on a
pipeline's lanes, as bench.py's loop does -- a prepared ctypes call per lane, batches of K calls and a join -- with the GPU
drained between batches so that no enqueue waits for room in a queue.  profiles/NOTES.md R6.13 did the same for one plan.

    python3 tools/pipeline_issue_time.py [workload] [calls_in_flight] [calls]      (defaults: cfgL 3 2000)

Prints one JSON line: microseconds per enqueue (median and mean over the batches, the join's share apart) and, for scale, the
time of a whole batch with its kernels (enqueue, join, synchronise)."""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import pollen_amd as pa  # noqa: E402
from pollen_amd import device as dev  # noqa: E402

WORKLOADS = {"cfgL": (1_000_000, 1000, 100_000, "pangenome"), "cfgM": (100_000, 100, 100_000, "pangenome"), "cfgS": (10_000, 100, 10_000, "pangenome")}  # (bench.py's)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfgL"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    S, P, L, model = WORKLOADS[name]
    steps, begins, ends, seg_len = pa.synth(1, S, P, L, model, False).soa()
    graph = dev.DeviceGraph(steps, begins, ends, S, seg_len)
    pipe = dev.DepthPipeline(graph, k)
    bufs = [torch.zeros(2 * S, dtype=torch.int32, device="cuda:0") for _ in range(k)]
    torch.cuda.synchronize()
    fn = dev._lib.lib().flatgfa_dev_pipeline_seg_depth
    none = ctypes.c_void_p(-1)
    prepared = [(lambda f=fn, p=pipe._p, d=ctypes.c_void_p(b[:S].data_ptr()), u=ctypes.c_void_p(b[S:].data_ptr()): f(p, d, u, none)) for b in bufs]
    for _ in range(3):  # (the first calls make the images; the description waits for them)
        for c in prepared:
            assert c() == 0, dev._lib.last_error()
        pipe.status()
    desc = pipe.describe()
    torch.cuda.synchronize()
    issue, join, whole = [], [], []
    now = time.perf_counter_ns
    for _ in range(calls // k):
        t0 = now()
        for c in prepared:
            c()
        t1 = now()
        pipe.join()
        t2 = now()
        torch.cuda.synchronize()
        t3 = now()
        issue.append((t1 - t0) / k)
        join.append(t2 - t1)
        whole.append(t3 - t0)
    pipe.status()
    us = 1e-3
    print(json.dumps({"workload": name, "calls_in_flight": k, "calls": len(issue) * k,
                      "issue_us_per_call": {"median": round(statistics.median(issue) * us, 2), "mean": round(statistics.fmean(issue) * us, 2),
                                            "p90": round(sorted(issue)[int(0.9 * len(issue))] * us, 2)},
                      "join_us_per_batch": {"median": round(statistics.median(join) * us, 2), "mean": round(statistics.fmean(join) * us, 2)},
                      "batch_us_enqueue_join_synchronise": {"median": round(statistics.median(whole) * us, 2)},
                      "plan": desc}))
    pipe.close()


if __name__ == "__main__":
    main()
