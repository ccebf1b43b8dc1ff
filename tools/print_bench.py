"""The GFA printer at scale, host and device: one JSON line.

    python tools/print_bench.py [--segs 1000000] [--paths 1000] [--steps 100000] [--chop 3] [--host-reps 2] [--out FILE]

Two inputs, in one sitting on one box: cfg-L (bench.py's graph: synth(1, 1 M segments, 1000 paths of 100 k steps)) and
cfg-L chopped at 3 (`--chop 0` leaves it out).  The single-thread C++ restatement of print.rs (tools/print_cpu.cpp, compiled
here with g++ -O3 -march=native) is first held against the host printer on small graphs, then gives the sha256 of each text;
no time is reported unless the host printer's and the device's texts have that sha256.  Per input, on the handle as it comes
(not resident) and again after to_device(0) (resident: the steps are read in place):

  host_ms      flatgfa_print_gfa, the whole call into its malloc'd buffer: best of --host-reps
  stream_ms    flatgfa_print_gfa_stream into a sink that counts: the whole call, best of 3 after one warm call
  buffer_ms    flatgfa_print_gfa_device into the malloc'd buffer, likewise
  bytes_ms     flatgfa_print_gfa_bytes: the open phase alone (checks, uploads, the count)
  kernel_ms    the kernels alone (HIP events: flatgfa_dev_profile_enable / _read), a sum per kernel name
  cpu_s        the restatement's own seconds, memory to memory, one thread
  pinned_ms    a pinned device-to-host copy of the text's bytes alone (torch; the rate of a gigabyte, times the bytes)

and the two ratios that matter: host_ms / stream_ms and stream_ms / pinned_ms.
"""
import argparse
import ctypes
import hashlib
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pollen_amd as pa  # noqa: E402
from pollen_amd import _lib  # noqa: E402


def build_cpu(work):
    so = os.path.join(work, "print_cpu.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "print_cpu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.print_cpu.restype = ctypes.c_int
    lib.print_cpu.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                              ctypes.POINTER(ctypes.c_double)]
    lib.print_cpu_free.argtypes = [ctypes.c_void_p]
    return lib


def view(ptr, n):
    return (ctypes.c_char * n).from_address(ptr) if n else b""


def sha(ptr, n):
    return hashlib.sha256(view(ptr, n)).hexdigest()


def run_cpu(cpu, g, keep=False):
    """The restatement on the handle's own pools (read in place): its sha256, bytes and seconds."""
    lib = _lib.lib()
    ptrs, lens = (ctypes.c_void_p * 11)(), (ctypes.c_uint64 * 11)()
    for ix in range(11):
        data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.flatgfa_pool(g._h, ix, ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
        ptrs[ix], lens[ix] = data.value, n.value
    text, n, secs = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_double()
    rc = cpu.print_cpu(ptrs, lens, ctypes.byref(text), ctypes.byref(n), ctypes.byref(secs))
    assert rc == 0, f"the restatement stopped ({rc})"
    out = {"sha": sha(text.value, n.value), "bytes": n.value, "s": secs.value, "text": bytes(view(text.value, n.value)) if keep else None}
    cpu.print_cpu_free(text)
    return out


def restatement_is_the_printer(cpu):
    import print_shapes as ps
    texts = list(ps.HANDMADE.values()) + [ps.digit_names(), ps.alternating(50), ps.long_overlaps(40)]
    for text in texts:
        with pa.parse_bytes(text) as g:
            assert run_cpu(cpu, g, True)["text"] == g.gfa_text(), "the restatement is not the printer"
    with pa.synth(3, 500, 7, 300, "pangenome", True) as g:
        assert run_cpu(cpu, g, True)["text"] == g.gfa_text(), "the restatement is not the printer"


def best_ms(n, fn):
    best = 1e18
    for _ in range(n):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return round(best * 1e3, 3)


def measure(g, want, host_reps):
    lib = _lib.lib()
    out = {}

    def host():
        p, k = ctypes.c_void_p(), ctypes.c_size_t()
        t0 = time.perf_counter()
        rc = lib.flatgfa_print_gfa(g._h, ctypes.byref(p), ctypes.byref(k))
        dt = time.perf_counter() - t0
        assert rc == 0, _lib.last_error()
        return p, k.value, dt
    best = 1e18
    for rep in range(host_reps):
        p, k, dt = host()
        best = min(best, dt)
        if rep == 0:
            assert (sha(p.value, k), k) == (want["sha"], want["bytes"]), "the host printer's text is not the restatement's"
        lib.flatgfa_free_text(p)
    out["host_ms"] = round(best * 1e3, 3)
    # the stream: first into a sink that hashes, then into one that counts
    h, seen = hashlib.sha256(), [0, 0]

    def hashing(_ctx, ptr, k):
        h.update(view(ptr, k))
        seen[0] += k
        return 0

    def counting(_ctx, ptr, k):
        seen[1] += k
        return 0
    t = time.perf_counter()
    assert lib.flatgfa_print_gfa_stream(g._h, _lib.SINK_T(hashing), None) == 0, _lib.last_error()
    out["first_call_ms_hashing_sink"] = round((time.perf_counter() - t) * 1e3, 1)
    assert (h.hexdigest(), seen[0]) == (want["sha"], want["bytes"]), "the device's text is not the restatement's: nothing is reported"
    count = _lib.SINK_T(counting)

    def stream():
        seen[1] = 0
        assert lib.flatgfa_print_gfa_stream(g._h, count, None) == 0, _lib.last_error()
        assert seen[1] == want["bytes"]
    out["stream_ms"] = best_ms(3, stream)

    def size():
        b = ctypes.c_uint64()
        assert lib.flatgfa_print_gfa_bytes(g._h, ctypes.byref(b)) == 0 and b.value == want["bytes"], _lib.last_error()
    out["bytes_ms"] = best_ms(3, size)
    best = 1e18
    for rep in range(3):
        p, k = ctypes.c_void_p(), ctypes.c_size_t()
        t0 = time.perf_counter()
        rc = lib.flatgfa_print_gfa_device(g._h, ctypes.byref(p), ctypes.byref(k))
        best = min(best, time.perf_counter() - t0)
        assert rc == 0, _lib.last_error()
        if rep == 2:
            assert sha(p.value, k.value) == want["sha"], "the device's buffer is not the restatement's"
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
    out["kernel_ms_sum"] = round(sum(per.values()), 3)
    out["kernel_launches"] = k
    tiles = per.get("print_tiles", 0.0)
    out["tiles_gbps_of_output"] = round(want["bytes"] / tiles / 1e6, 1) if tiles else None
    out["stream_gbps"] = round(want["bytes"] / out["stream_ms"] / 1e6, 2)
    out["host_over_stream"] = round(out["host_ms"] / out["stream_ms"], 2)
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
    res = {"what": "the GFA printer, host (flatgfa_print_gfa) and device (flatgfa_print_gfa_stream / _device)",
           "graph": f"synth(1, {args.segs}, {args.paths}, {args.steps}, pangenome)", "box": {"cpu": platform.processor() or platform.machine(), "cpus": os.cpu_count()}}
    with tempfile.TemporaryDirectory(prefix="print_bench_") as work:
        cpu = build_cpu(work)
        restatement_is_the_printer(cpu)
        res["restatement_matches_host_printer"] = True
        if pa.device_count() < 1:
            raise SystemExit("print_bench: no HIP device is visible; nothing is measured without one")
        import torch
        res["box"]["gpu"] = torch.cuda.get_device_name(0)
        res["box"]["torch"], res["box"]["hip"] = torch.__version__, torch.version.hip
        res["box"]["library_head"] = open(os.path.join(ROOT, "pollen_amd", "lib", "HEAD")).read() if os.path.exists(os.path.join(ROOT, "pollen_amd", "lib", "HEAD")) else None
        n = 1 << 30
        d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        h = torch.empty(n, dtype=torch.uint8, pin_memory=True)

        def copy():
            h.copy_(d, non_blocking=True)
            torch.cuda.synchronize()
        copy()
        gbps = n / best_ms(3, copy) / 1e6
        res["pinned_d2h_gbps"] = round(gbps, 1)
        del d, h
        torch.cuda.empty_cache()
        base = pa.synth(1, args.segs, args.paths, args.steps, "pangenome", False)
        inputs = [("cfgL", base)]
        if args.chop:
            inputs.append((f"cfgL_chop{args.chop}", base.chop(args.chop)))
        for key, g in inputs:
            want = run_cpu(cpu, g)
            n_steps = ctypes.c_uint64()
            assert _lib.lib().flatgfa_pool(g._h, 4, None, ctypes.byref(n_steps), None) == 0
            one = {"steps": n_steps.value, "segments": g.segment_count,
                   "text_bytes": want["bytes"], "sha256": want["sha"], "cpu_single_thread_s": round(want["s"], 3),
                   "pinned_ms": round(want["bytes"] / gbps / 1e6, 3)}
            one["not_resident"] = measure(g, want, args.host_reps)
            g.to_device(0)
            one["resident"] = measure(g, want, 1)
            for where in ("not_resident", "resident"):
                one[where]["stream_over_pinned"] = round(one[where]["stream_ms"] / one["pinned_ms"], 2)
            res[key] = one
            print(json.dumps({key: one}), file=sys.stderr, flush=True)
            g.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
