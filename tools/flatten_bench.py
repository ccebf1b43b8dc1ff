"""Flatten at scale: one JSON line.

    python tools/flatten_bench.py [--segs 1000000] [--paths 1000] [--steps 100000] [--out FILE]

The cfg-L graph with sequences (synth(1, 1 M segments, 1000 paths of 100 k steps)): 100 M BED lines.  The single-thread C++
restatement of flatten.py (tools/flatten_cpu.cpp, compiled here with g++ -O3 -march=native) stands in for the reference --
it is first held against tests/flatten_model.py on a small graph -- and gives the sha256 of both texts; no time is reported
unless the GPU's texts have the same sha256, before and after timing.  Then, for the BED and the FASTA each:

  sink_ms      flatgfa_flatten_stream into a sink that discards: the whole call, best of 3 after one warm call
  buffer_ms    flatgfa_flatten_bed / _fasta into the malloc'd buffer, likewise
  kernel_ms    the kernels alone, on the device-resident pieces they write (HIP events: flatgfa_dev_profile_enable / _read), as
               a sum per kernel name, and the GB/s of output that is
  cpu_s        the restatement's own seconds, memory to memory, one thread
  pinned_d2h   a pinned device-to-host copy of a gigabyte (torch), for the expectation that the whole call is bound by the copy
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pollen_amd as pa  # noqa: E402
from pollen_amd import _lib  # noqa: E402

NAME = b"cfgL.og"


def build_cpu(work):
    so = os.path.join(work, "flatten_cpu.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "flatten_cpu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.flatten_cpu.restype = ctypes.c_int
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.flatten_cpu.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, vp, ctypes.c_char_p, ctypes.c_size_t,
                                ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t),
                                ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.flatten_cpu_free.argtypes = [ctypes.c_void_p]
    return lib


def view(ptr, n):
    return (ctypes.c_char * n).from_address(ptr) if n else b""


def run_cpu(lib, pools, name):
    """(sha256 of the FASTA, of the BED, their lengths, the restatement's seconds); `keep` returns the texts too."""
    segs, paths = pools["segs"], pools["paths"]
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    arrs = [c(segs["seq_start"], np.uint32), c(segs["seq_end"] - segs["seq_start"], np.uint32), c(pools["seq_data"], np.uint8),
            c(pools["steps"], np.uint32), c(paths["steps_start"], np.uint32), c(paths["steps_end"], np.uint32),
            c(paths["name_start"], np.uint32), c(paths["name_end"], np.uint32), c(pools["name_data"], np.uint8)]
    fa, bed = ctypes.c_void_p(), ctypes.c_void_p()
    nf, nb = ctypes.c_size_t(), ctypes.c_size_t()
    sf, sb = ctypes.c_double(), ctypes.c_double()
    p = [a.ctypes.data for a in arrs]
    rc = lib.flatten_cpu(p[0], p[1], len(segs), p[2], p[3], p[4], p[5], p[6], p[7], len(paths), p[8], name, len(name),
                         ctypes.byref(fa), ctypes.byref(nf), ctypes.byref(bed), ctypes.byref(nb), ctypes.byref(sf), ctypes.byref(sb))
    assert rc == 0, "the restatement ran out of memory"
    out = {"fasta": bytes(view(fa.value, nf.value)) if nf.value < (1 << 24) else None, "bed": bytes(view(bed.value, nb.value)) if nb.value < (1 << 24) else None,
           "fasta_sha": hashlib.sha256(view(fa.value, nf.value)).hexdigest(), "bed_sha": hashlib.sha256(view(bed.value, nb.value)).hexdigest(),
           "fasta_bytes": nf.value, "bed_bytes": nb.value, "fasta_s": sf.value, "bed_s": sb.value}
    lib.flatten_cpu_free(fa)
    lib.flatten_cpu_free(bed)
    return out


def restatement_is_the_model(cpu):
    """The restatement on a small graph against tests/flatten_model.py (itself held against `slow_odgi flatten`'s bytes)."""
    import chop_model as cm
    import flatten_model as fm
    with pa.synth(3, 500, 7, 300, "pangenome", True) as g:
        p = cm.pools_of(g)
        got = run_cpu(cpu, {n: getattr(p, n) for n in ("segs", "paths", "seq_data", "steps", "name_data")}, b"small.og")
        assert got["fasta"] == fm.fasta(p, b"small.og") and got["bed"] == fm.bed(p, b"small.og"), "the restatement is not flatten.py"


def gpu_sha(g, what):
    h, n = hashlib.sha256(), [0]

    def sink(_ctx, ptr, k):
        h.update(view(ptr, k))
        n[0] += k
        return 0
    rc = _lib.lib().flatgfa_flatten_stream(g._h, NAME, len(NAME), what, _lib.SINK_T(sink), None)
    assert rc == 0, _lib.last_error()
    return h.hexdigest(), n[0]


def best_ms(n, fn):
    best = 1e18
    for _ in range(n):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return round(best * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=1_000_000)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.lib()
    res = {"what": "flatten (fgfa flatten)", "graph": f"synth(1, {args.segs}, {args.paths}, {args.steps}, pangenome, with sequences)", "name": NAME.decode()}
    with tempfile.TemporaryDirectory(prefix="flatten_bench_") as work:
        cpu = build_cpu(work)
        restatement_is_the_model(cpu)
        res["restatement_matches_model"] = True
        if pa.device_count() < 1:
            raise SystemExit("flatten_bench: no HIP device is visible; nothing is measured without one")
        import torch
        g = pa.synth(1, args.segs, args.paths, args.steps, "pangenome", True)
        want = run_cpu(cpu, {n: g.pool(n) for n in ("segs", "paths", "seq_data", "steps", "name_data")}, NAME)
        res.update(lines=args.paths * args.steps, fasta_bytes=want["fasta_bytes"], bed_bytes=want["bed_bytes"],
                   fasta_sha256=want["fasta_sha"], bed_sha256=want["bed_sha"],
                   cpu_single_thread_s={"fasta": round(want["fasta_s"], 3), "bed": round(want["bed_s"], 3)})
        discard = _lib.SINK_T(lambda ctx, p, n: 0)
        for key, what, call in (("fasta", 1, lib.flatgfa_flatten_fasta), ("bed", 2, lib.flatgfa_flatten_bed)):
            t = time.perf_counter()
            sha, n = gpu_sha(g, what)  # (the first call: the legend, the uploads)
            first_ms = round((time.perf_counter() - t) * 1e3, 1)
            assert (sha, n) == (want[key + "_sha"], want[key + "_bytes"]), f"the GPU's {key} is not the restatement's: nothing is reported"
            out = {"first_call_ms_hashing_sink": first_ms}

            def stream():
                assert lib.flatgfa_flatten_stream(g._h, NAME, len(NAME), what, discard, None) == 0, _lib.last_error()
            out["sink_ms"] = best_ms(3, stream)
            def buffer():
                p, k = ctypes.c_void_p(), ctypes.c_size_t()
                t0 = time.perf_counter()
                rc = call(g._h, NAME, len(NAME), ctypes.byref(p), ctypes.byref(k))
                dt = time.perf_counter() - t0
                assert rc == 0, _lib.last_error()
                return p, k.value, dt
            best = 1e18
            for rep in range(3):
                p, k, dt = buffer()
                best = min(best, dt)
                if rep == 2:
                    assert hashlib.sha256(view(p.value, k)).hexdigest() == want[key + "_sha"], f"the GPU's {key} buffer is not the restatement's"
                lib.flatgfa_free_text(p)
            out["buffer_ms"] = round(best * 1e3, 3)
            # the kernels alone
            lib.flatgfa_dev_profile_enable(1)
            stream()
            cap = 1 << 16
            names, ms = (ctypes.c_char_p * cap)(), (ctypes.c_float * cap)()
            k = lib.flatgfa_dev_profile_read(names, ms, cap)
            lib.flatgfa_dev_profile_enable(0)
            per = {}
            for i in range(k):
                nm = names[i].decode()
                per[nm] = per.get(nm, 0.0) + ms[i]
            out["kernel_ms"] = {a: round(b, 3) for a, b in sorted(per.items())}
            out["kernel_launches"] = k
            body = per.get("flatten_" + key, 0.0)
            out["kernel_gbps_of_output"] = round(want[key + "_bytes"] / body / 1e6, 1) if body else None
            out["sink_gbps"] = round(want[key + "_bytes"] / out["sink_ms"] / 1e6, 2)
            out["buffer_gbps"] = round(want[key + "_bytes"] / out["buffer_ms"] / 1e6, 2)
            sha, n = gpu_sha(g, what)
            assert (sha, n) == (want[key + "_sha"], want[key + "_bytes"]), f"the GPU's {key} changed while it was timed"
            out["sha256_matches_restatement"] = True
            res[key] = out
        g.close()
        # the copy the whole call is expected to be bound by
        n = 1 << 30
        d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        h = torch.empty(n, dtype=torch.uint8, pin_memory=True)

        def copy():
            h.copy_(d, non_blocking=True)
            torch.cuda.synchronize()
        copy()
        res["pinned_d2h_gbps"] = round(n / best_ms(3, copy) / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
