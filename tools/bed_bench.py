"""BED intersection at scale: one JSON line.

    python tools/bed_bench.py [--a-lines 10000000] [--b-lines 1000000] [--nested-scale 1] [--out FILE]

Two synthetic shapes over 24 names, both files sorted by name and start:

  disjoint   --a-lines A intervals of 140 bases, one every 10, against --b-lines disjoint B intervals of 60 bases, one every 100:
             an A interval meets (140 + 60) / 100 = 2 of them on average
  nested     the same with one long B interval per name in front of the short ones.  Every A entry's candidate range then
             begins at its group's head -- the running maximum of `end` is the long interval's everywhere, which is what it is
             kept for -- so the candidates grow with the square of the size (1.9 * 10^11 at the default sizes: the restatement
             alone takes over a minute); --nested-scale N runs this shape at 1 / N of both line counts

The single-thread C++ restatement (tools/bed_cpu.cpp, compiled here with g++ -O3 -march=native: the same grouping and
bisection, not the reference's double loop) gives the sha256 of each text; no time is reported unless the device's text has
that sha256 before and after the timing.  Per shape:

  stream_ms    flatgfa_bed_intersect_stream, host buffers to a sink that counts: the whole call, best of 3 after one warm call
  count_ms     flatgfa_bed_intersect_count: the same without the text kernels and the text's download
  kernel_ms    the kernels alone (HIP events: flatgfa_dev_profile_enable / _read), a sum per kernel name
  pinned_ms    pinned copies alone of as many bytes as both inputs (host to device) and the output (device to host): the floor
  cpu_s        the restatement's own seconds, memory to memory, one thread: parse, intern and group, intersect and print

and the two ratios: cpu over stream, stream over pinned.
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

NAMES = 24


def build_cpu(work):
    so = os.path.join(work, "bed_cpu.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "bed_cpu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.bed_cpu.restype = ctypes.c_int
    lib.bed_cpu.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                            ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    lib.bed_cpu_free.argtypes = [ctypes.c_void_p]
    lib.bed_synth.restype = ctypes.c_size_t
    lib.bed_synth.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    return lib


def view(ptr, n):
    return (ctypes.c_char * n).from_address(ptr) if n else b""


def run_cpu(cpu, a: bytes, b: bytes, keep=False):
    """The restatement: its text's sha256 and size, (lines, bytes, candidates, unsorted groups), its seconds by phase."""
    text, n = ctypes.c_void_p(), ctypes.c_size_t()
    stats, secs = (ctypes.c_uint64 * 4)(), (ctypes.c_double * 3)()
    rc = cpu.bed_cpu(a, len(a), b, len(b), ctypes.byref(text), ctypes.byref(n), stats, secs)
    assert rc == 0, f"the restatement stopped ({rc})"
    out = {"sha": hashlib.sha256(view(text.value, n.value)).hexdigest(), "bytes": n.value, "stats": tuple(stats), "s": list(secs),
           "text": bytes(view(text.value, n.value)) if keep else None}
    cpu.bed_cpu_free(text)
    return out


def synth(cpu, per_name, at, step, width, front_end=0) -> bytes:
    buf = ctypes.create_string_buffer(cpu.bed_synth(None, NAMES, per_name, at, step, width, front_end))
    n = cpu.bed_synth(buf, NAMES, per_name, at, step, width, front_end)
    return buf.raw[:n]


def best_ms(n, fn):
    best = 1e18
    for _ in range(n):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return round(best * 1e3, 3)


def measure(a, b, want, rates):
    lib = _lib.lib()
    out = {}

    def hashed():
        h, seen = hashlib.sha256(), [0]

        def sink(_ctx, ptr, k):
            h.update(view(ptr, k))
            seen[0] += k
            return 0
        t = time.perf_counter()
        assert lib.flatgfa_bed_intersect_stream(a, len(a), b, len(b), _lib.SINK_T(sink), None) == 0, _lib.last_error()
        ms = round((time.perf_counter() - t) * 1e3, 1)
        assert (h.hexdigest(), seen[0]) == (want["sha"], want["bytes"]), "the device's text is not the restatement's: nothing is reported"
        return ms
    out["first_call_ms_hashing_sink"] = hashed()
    seen = [0]

    def counting(_ctx, ptr, k):
        seen[0] += k
        return 0
    count = _lib.SINK_T(counting)

    def stream():
        seen[0] = 0
        assert lib.flatgfa_bed_intersect_stream(a, len(a), b, len(b), count, None) == 0, _lib.last_error()
        assert seen[0] == want["bytes"]
    out["stream_ms"] = best_ms(3, stream)

    def counts():
        u = [ctypes.c_uint64() for _ in range(4)]
        assert lib.flatgfa_bed_intersect_count(a, len(a), b, len(b), *[ctypes.byref(x) for x in u]) == 0, _lib.last_error()
        assert tuple(x.value for x in u) == want["stats"], "the device's counts are not the restatement's"
    out["count_ms"] = best_ms(3, counts)
    lib.flatgfa_dev_profile_enable(1)
    stream()
    cap = 1 << 18
    names, ms = (ctypes.c_char_p * cap)(), (ctypes.c_float * cap)()
    k = lib.flatgfa_dev_profile_read(names, ms, cap)
    lib.flatgfa_dev_profile_enable(0)
    per = {}
    for i in range(k):
        nm = names[i].decode()
        per[nm] = per.get(nm, 0.0) + ms[i]
    out["kernel_ms"] = {x: round(y, 3) for x, y in sorted(per.items())}
    out["kernel_ms_sum"] = round(sum(per.values()), 3)
    out["kernel_scopes"] = k
    hashed()  # (and after the timing)
    out["text_checked_before_and_after"] = True
    out["pinned_ms"] = round((len(a) + len(b)) / rates[0] / 1e6 + want["bytes"] / rates[1] / 1e6, 3)
    out["cpu_over_stream"] = round(sum(want["s"]) * 1e3 / out["stream_ms"], 2)
    out["stream_over_pinned"] = round(out["stream_ms"] / out["pinned_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a-lines", type=int, default=10_000_000)
    ap.add_argument("--b-lines", type=int, default=1_000_000)
    ap.add_argument("--nested-scale", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"what": "BED intersection (flatgfa_bed_intersect_stream) beside a single-thread restatement of the same method and a pinned copy",
           "box": {"cpu": platform.processor() or platform.machine(), "cpus": os.cpu_count()}}
    with tempfile.TemporaryDirectory(prefix="bed_bench_") as work:
        cpu = build_cpu(work)
        if pa.device_count() < 1:
            raise SystemExit("bed_bench: no HIP device is visible; nothing is measured without one")
        import torch
        res["box"]["gpu"] = torch.cuda.get_device_name(0)
        res["box"]["torch"], res["box"]["hip"] = torch.__version__, torch.version.hip
        head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
        res["box"]["library_head"] = open(head).read() if os.path.exists(head) else None
        n = 1 << 28
        d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        h = torch.empty(n, dtype=torch.uint8, pin_memory=True)

        def sync(fn):
            fn()
            torch.cuda.synchronize()
        sync(lambda: h.copy_(d, non_blocking=True))
        rates = (n / best_ms(3, lambda: sync(lambda: d.copy_(h, non_blocking=True))) / 1e6,
                 n / best_ms(3, lambda: sync(lambda: h.copy_(d, non_blocking=True))) / 1e6)
        res["pinned_h2d_gbps"], res["pinned_d2h_gbps"] = round(rates[0], 1), round(rates[1], 1)
        del d, h
        torch.cuda.empty_cache()
        for key, scale, nested in (("disjoint", 1, False), ("nested", max(args.nested_scale, 1), True)):
            a_per, b_per = args.a_lines // scale // NAMES, args.b_lines // scale // NAMES
            span = b_per * 100
            a = synth(cpu, a_per, 0, max(span // max(a_per, 1), 1), 140)
            b = synth(cpu, b_per, 20, 100, 60, span + 1000 if nested else 0)
            want = run_cpu(cpu, a, b)
            one = {"a_lines": a.count(b"\n"), "b_lines": b.count(b"\n"), "a_bytes": len(a), "b_bytes": len(b), "text_bytes": want["bytes"],
                   "lines": want["stats"][0], "candidates": want["stats"][2], "unsorted_groups": want["stats"][3],
                   "hits_per_a_line": round(want["stats"][0] / max(a.count(b"\n"), 1), 3), "sha256": want["sha"],
                   "cpu_s": {"parse": round(want["s"][0], 3), "group": round(want["s"][1], 3), "intersect_and_print": round(want["s"][2], 3),
                             "all": round(sum(want["s"]), 3)}}
            one.update(measure(a, b, want, rates))
            res[key] = one
            print(json.dumps({key: one}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
