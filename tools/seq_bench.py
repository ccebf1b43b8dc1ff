"""The packed-sequence codec at scale: one JSON document (profiles/seq_bench.json).

    python tools/seq_bench.py [--bytes 2147483648] [--host-bytes 1073741824] [--out FILE]

Two parts, on one device in one run:

  resident    a device-made text of --bytes bytes: random A C T G in lines of 60 and a newline, as a FASTA body.  The pack's
              count, scan and fill kernels and the unpack kernel by their HIP events (flatgfa_dev_profile_enable / _read;
              median, min and max of --reps calls after --warm warm ones), each as bytes per second of its own traffic (count
              reads N; fill reads N and writes N / 2; unpack reads N / 2 and writes N, N the bases there) and as a multiple of
              a device-to-device copy of the same text timed in the same run.  Checked on the device before and after the
              timed calls: unpack(pack(text)) is the text without its newlines, and the count is theirs.
  host        the first --host-bytes of that text in host memory: flatgfa_seq_export to a file image and flatgfa_seq_import
              back (median, min, max of --host-reps calls after a warm one), beside the route's floor -- a pinned host-to-device
              copy of the text and a pinned device-to-host copy of the packed bytes, and the reverse pair, alone -- and beside
              the single-thread C++ restatement (tools/seq_cpu.cpp, g++ -O3 -march=native; its own seconds, memory to memory).
              The sha256 of the image and of the bases must equal the restatement's, or no time is reported."""
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
from pollen_amd import _lib  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

LINE = 61


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sha_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 26), b""):
            h.update(piece)
    return h.hexdigest()


def make_text(n):
    import torch
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(18)
    letters = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=d)
    text = letters[torch.randint(0, 4, (n,), generator=g, device=d)]
    text[LINE - 1::LINE] = ord("\n")
    return text


def device_events(fn, warm, reps):
    import torch
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return out


def resident(args):
    import torch
    text = make_text(args.bytes)
    n = int(text.numel())
    bases = n - n // LINE

    def check():
        packed, got = pdev.seq_pack(text)
        letters = pdev.seq_unpack(packed, got)
        # (the newlines are where make_text put them: whole lines as rows, then the last, unfinished line)
        rows = n // LINE
        ok = got == bases and bool(torch.equal(letters[:rows * (LINE - 1)].view(rows, LINE - 1), text[:rows * LINE].view(rows, LINE)[:, :LINE - 1]))
        ok = ok and bool(torch.equal(letters[rows * (LINE - 1):], text[rows * LINE:]))
        return ok, packed
    ok_before, packed = check()
    for _ in range(args.warm):
        pdev.seq_pack(text)
        pdev.seq_unpack(packed, bases)
    torch.cuda.synchronize()
    per = {}
    pdev.profile_enable(True)
    pdev.profile_read()
    for _ in range(args.reps):
        pdev.seq_pack(text)
        pdev.seq_unpack(packed, bases)
        torch.cuda.synchronize()
        got = {}
        for k, ms in pdev.profile_read():
            got[k] = got.get(k, 0.0) + ms
        for k, ms in got.items():
            per.setdefault(k, []).append(ms)
    pdev.profile_enable(False)
    ok_after, _ = check()
    dst = torch.empty_like(text)
    copy = device_events(lambda: dst.copy_(text), args.warm, args.reps)
    del dst
    res = {"text_bytes": n, "bases": bases, "packed_bytes": int(packed.numel()), "checked_before": ok_before, "checked_after": ok_after}
    if not (ok_before and ok_after):
        res["error"] = "unpack(pack(text)) is not the text without its newlines: no time reported"
        return res, text
    med = {k: statistics.median(v) for k, v in per.items()}
    cp = statistics.median(copy)
    traffic = {"seq_pack_count": n, "seq_pack_fill": n + bases // 2, "seq_unpack": bases // 2 + bases}
    res["kernels_ms"] = {k: stats(v) for k, v in sorted(per.items())}
    res["traffic_bytes"] = traffic
    res["GBps"] = {k: round(traffic[k] / med[k] / 1e6, 1) for k in traffic}
    res["d2d_copy_ms"] = stats(copy)
    res["d2d_copy_GBps"] = round(2 * n / cp / 1e6, 1)
    res["ratio_to_copy"] = {k: round(med[k] / cp, 3) for k in traffic}
    res["ratio_to_copy"]["pack_count_scan_fill"] = round((med["seq_pack_count"] + med["seq_pack_scan"] + med["seq_pack_fill"]) / cp, 3)
    res["floor_ratio_by_bytes"] = {k: round(traffic[k] / (2 * n), 3) for k in traffic}
    res["floor_ratio_by_bytes"]["pack_count_scan_fill"] = round((traffic["seq_pack_count"] + traffic["seq_pack_fill"]) / (2 * n), 3)
    return res, text


def wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def host(args, text, tool, work):
    import torch
    lib = _lib.lib()
    n = min(args.host_bytes, int(text.numel()))
    h_text = text[:n].cpu().numpy().tobytes()
    src, img, back = (os.path.join(work, x) for x in ("text.bin", "image.bin", "bases.bin"))
    with open(src, "wb") as f:
        f.write(h_text)
    r = subprocess.run([tool, "export", src, img], check=True, capture_output=True)
    cpu_bases, cpu_export_s = int(r.stdout.split()[0]), float(r.stdout.split()[1])
    r = subprocess.run([tool, "import", img, back], check=True, capture_output=True)
    cpu_import_s = float(r.stdout.split()[1])
    cpu_image_sha, cpu_bases_sha = sha_file(img), sha_file(back)
    for p in (src, img, back):
        os.unlink(p)

    def export():
        p, m = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib.flatgfa_seq_export(h_text, n, ctypes.byref(p), ctypes.byref(m))
        assert rc == 0, _lib.last_error()
        return p, m

    def take(p, m):
        b = bytes((ctypes.c_char * m.value).from_address(p.value))
        lib.flatgfa_free_text(p)
        return b
    image = take(*export())
    res = {"text_bytes": n, "bases": cpu_bases, "image_bytes": len(image), "sha256_image_cpu": cpu_image_sha,
           "sha256_image": hashlib.sha256(image).hexdigest(), "sha256_bases_cpu": cpu_bases_sha, "cpu_export_s": cpu_export_s,
           "cpu_import_s": cpu_import_s}

    def imp():
        p, m = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib.flatgfa_seq_import(image, len(image), ctypes.byref(p), ctypes.byref(m))
        assert rc == 0, _lib.last_error()
        return p, m
    res["sha256_bases"] = hashlib.sha256(take(*imp())).hexdigest()
    if res["sha256_image"] != cpu_image_sha or res["sha256_bases"] != cpu_bases_sha:
        res["error"] = "the library's bytes are not the restatement's: no time reported"
        return res
    res["seq_export_ms"] = stats(wall(lambda: lib.flatgfa_free_text(export()[0]), args.host_reps))
    res["seq_import_ms"] = stats(wall(lambda: lib.flatgfa_free_text(imp()[0]), args.host_reps))
    # the floor: the same bytes over PCIe from and to pinned memory, nothing else
    pin_text = torch.from_numpy(np.frombuffer(h_text, np.uint8).copy()).pin_memory()
    pin_packed = torch.empty(cpu_bases // 2 + 1, dtype=torch.uint8).pin_memory()
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_packed = torch.empty(cpu_bases // 2 + 1, dtype=torch.uint8, device="cuda:0")

    def pair(up_dst, up_src, down_dst, down_src):
        up_dst.copy_(up_src, non_blocking=True)
        down_dst.copy_(down_src, non_blocking=True)
        torch.cuda.synchronize()
    res["pinned_text_up_packed_down_ms"] = stats(wall(lambda: pair(d_text, pin_text, pin_packed, d_packed), args.host_reps))
    res["pinned_packed_up_text_down_ms"] = stats(wall(lambda: pair(d_packed, pin_packed, pin_text[:cpu_bases], d_text[:cpu_bases]), args.host_reps))
    res["export_over_floor"] = round(res["seq_export_ms"]["median"] / res["pinned_text_up_packed_down_ms"]["median"], 2)
    res["import_over_floor"] = round(res["seq_import_ms"]["median"] / res["pinned_packed_up_text_down_ms"]["median"], 2)
    res["export_speedup_over_cpu"] = round(cpu_export_s * 1e3 / res["seq_export_ms"]["median"], 2)
    res["import_speedup_over_cpu"] = round(cpu_import_s * 1e3 / res["seq_import_ms"]["median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 31)
    ap.add_argument("--host-bytes", type=int, default=1 << 30)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("seq_bench: no device: nothing is measured without one")
    with tempfile.TemporaryDirectory() as work:
        tool = os.path.join(work, "seq_cpu")
        subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", os.path.join(ROOT, "tools", "seq_cpu.cpp"), "-o", tool])
        head = os.path.join(ROOT, "pollen_amd", "lib", "HEAD")
        res = {"what": "the packed-sequence codec (fgfa seq-export, seq-import)", "device": torch.cuda.get_device_name(0),
               "build": open(head).read() if os.path.exists(head) else "unknown", "warm": args.warm, "reps": args.reps, "host_reps": args.host_reps}
        res["resident"], text = resident(args)
        res["host"] = host(args, text, tool, work)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
