"""The GAF lookup at scale: one JSON line.

    python tools/gaf_lookup_bench.py [--gb 1] [--workdir DIR] [--out FILE] [--skip-cli]

A seeded GAF of --gb gigabytes over the cfg-L graph with sequences (synth(1, 1 M segments, 1000 paths of 100 k steps)), made
as tools/pangenotype_bench.py makes its own -- short-read-like lines with a path field of 5-20 nodes -- with `start` a
quarter and `end` three quarters of the way along each walk (six digits each, zero-padded).  The single-thread C++
restatement of gaf.rs (tools/gaf_lookup_cpu.cpp, compiled here with g++ -O3 -march=native) stands in for the reference; every
timed output is compared with its text before and after timing.  Then:

  (a) a_kernel     flatgfa_dev_gaf_count + _fill (events and the `-s` text) on device-resident text, wall time around the
                   two calls and a device wait, warm, best of 5; GB/s of input + output bytes
  (b) b_end_to_end flatgfa_gaf_seqs, host buffer to host text, best of 3, beside the restatement's own seconds (memory to
                   memory, one thread) and a pinned copy of the same input (up) and output (down) bytes.  THE GATE: faster
                   than the restatement.
  (c) c_cli        `fgfa -i cfgL.flatgfa gaf GAF -s` and `-b`, whole processes, beside the restatement's processes
  (d) long_line    one read of a million tokens (a line of 8 MB): flatgfa_gaf_seqs beside the restatement
"""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pollen_amd as pa  # noqa: E402
from pollen_amd import _lib  # noqa: E402

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
BLOCK = 65536
DIGITS = 7


def gaf_block(rng, names, seg_len, first_read, n_tok):
    """BLOCK lines of n_tok nodes each as a (BLOCK, width) uint8 array."""
    head = b"r%010d\t150\t0\t150\t+\t"
    tail = np.frombuffer(b"\t5000\t000000\t000000\t148\t150\t60\tNM:i:2\tAS:f:140\tdv:f:0.013\tid:f:0.987\tcg:Z:150M\n", dtype=np.uint8)
    hw = len(head % 0)
    pw = n_tok * (DIGITS + 1)
    a = np.empty((BLOCK, hw + pw + len(tail)), dtype=np.uint8)
    rid = np.arange(first_read, first_read + BLOCK, dtype=np.int64)
    a[:, :hw] = np.frombuffer(head % 0, dtype=np.uint8)
    for d in range(10):
        a[:, 10 - d] = (rid // 10 ** d % 10).astype(np.uint8) + ord("0")
    a[:, hw + pw:] = tail
    ids = rng.integers(0, len(names), size=(BLOCK, n_tok), dtype=np.int64)
    tok = a[:, hw:hw + pw].reshape(BLOCK, n_tok, DIGITS + 1)
    tok[:, :, 0] = np.where(rng.random((BLOCK, n_tok)) < 0.5, ord(">"), ord("<"))
    v = names[ids]
    for d in range(DIGITS, 0, -1):
        tok[:, :, d] = (v % 10).astype(np.uint8) + ord("0")
        v = v // 10
    total = seg_len[ids].sum(axis=1)
    assert int(total.max()) < 10 ** 6
    for col, val in ((hw + pw + 6, total // 4), (hw + pw + 13, total - total // 4)):  # start and end, inside the walk
        for d in range(6):
            a[:, col + 5 - d] = (val // 10 ** d % 10).astype(np.uint8) + ord("0")
    return a


def best_of(n, fn):
    best, out = 1e9, None
    for _ in range(n):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    args = ap.parse_args()
    import torch
    work = args.workdir or tempfile.mkdtemp(prefix="gaf_lookup_bench_")
    os.makedirs(work, exist_ok=True)
    res = {"what": "GAF lookup (fgfa gaf) over cfg-L", "graph": "synth(1, 1000000, 1000, 100000, pangenome, with sequences)"}
    try:
        t = time.perf_counter()
        g = pa.synth(1, 1_000_000, 1000, 100_000, "pangenome", True)
        segs = g.pool("segs")
        names = np.asarray(segs["name"], dtype=np.uint64)
        seq_start = np.asarray(segs["seq_start"], dtype=np.uint32)
        seg_len = (np.asarray(segs["seq_end"], dtype=np.int64) - seq_start).astype(np.int64)
        assert names.max() < 10 ** DIGITS
        gaf = os.path.join(work, "reads.gaf")
        rng = np.random.default_rng(1)
        nbytes, reads = 0, 0
        with open(gaf, "wb") as f:
            while nbytes < args.gb * (1 << 30):
                a = gaf_block(rng, names, seg_len, reads, int(rng.integers(5, 21)))
                f.write(a.tobytes())
                nbytes += a.size
                reads += BLOCK
        res.update(gaf_bytes=nbytes, reads=reads, generate_s=round(time.perf_counter() - t, 1))
        text = np.fromfile(gaf, dtype=np.uint8)  # anonymous memory, not the mapping

        # the restatement's answer: what everything below is compared with
        files = {}
        for nm, arr in (("names.u64", names.astype("<u8")), ("seq_start.u32", seq_start.astype("<u4")),
                        ("seq_len.u32", seg_len.astype("<u4")), ("seq.bin", np.asarray(g.pool("seq_data"), dtype=np.uint8))):
            files[nm] = os.path.join(work, nm)
            arr.tofile(files[nm])
        cpu = os.path.join(work, "gaf_lookup_cpu")
        subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", os.path.join(ROOT, "tools", "gaf_lookup_cpu.cpp"), "-o", cpu])
        cpu_args = [cpu, files["names.u64"], files["seq_start.u32"], files["seq_len.u32"], files["seq.bin"]]
        want_file = os.path.join(work, "want.txt")

        def run_cpu(gaf_path, out_path):
            t0 = time.perf_counter()
            r = subprocess.run(cpu_args + [gaf_path, "-s", out_path], capture_output=True, check=True, timeout=3000)
            return time.perf_counter() - t0, float(re.search(rb"lookup_seconds=([0-9.]+)", r.stderr).group(1))
        cpu_best, cpu_proc = 1e9, 1e9
        for _ in range(2):
            proc_s, inner_s = run_cpu(gaf, want_file)
            cpu_best, cpu_proc = min(cpu_best, inner_s), min(cpu_proc, proc_s)
        want = np.fromfile(want_file, dtype=np.uint8)
        out_bytes = int(want.size)
        res.update(seq_text_bytes=out_bytes)
        got = np.frombuffer(g.gaf_seqs(memoryview(text)), dtype=np.uint8)
        assert got.size == want.size and (got == want).all(), "flatgfa_gaf_seqs differs from the restatement"
        res["text_matches_restatement"] = True

        # (a) the kernels on device-resident text, through the device entry
        lib = _lib.lib()
        dev = torch.device("cuda:0")
        kern = {}
        job = ctypes.c_void_p()
        for size in (64 << 20, 512 << 20):
            if size > nbytes:
                continue
            n = int(np.flatnonzero(text[:size] == 10)[-1]) + 1
            d = torch.from_numpy(text[:n]).to(dev)
            nl, ne, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            out = None
            best = 1e9
            for rep in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = lib.flatgfa_dev_gaf_count(g._h, d.data_ptr(), n, 1, None, ctypes.byref(job), ctypes.byref(nl), ctypes.byref(ne), ctypes.byref(nb))
                assert rc == 0, _lib.last_error()
                if out is None:
                    out = torch.empty(nb.value, dtype=torch.uint8, device=dev)
                rc = lib.flatgfa_dev_gaf_fill(job, None, None, None, None, None, None, None, out.data_ptr(), None)
                assert rc == 0, _lib.last_error()
                torch.cuda.synchronize()
                if rep:
                    best = min(best, time.perf_counter() - t0)
            o = out.cpu().numpy()
            assert (o == want[:o.size]).all(), "the device entry's text differs from the restatement"
            kern[f"{n >> 20}MB"] = {"ms": round(best * 1e3, 3), "out_bytes": int(nb.value), "events": int(ne.value),
                                    "gbps_in_plus_out": round((n + nb.value) / best / 1e9, 1)}
            del d, out
        lib.flatgfa_dev_gaf_free(job)
        res["a_kernel"] = kern
        torch.cuda.empty_cache()

        # (b) host buffer -> host text: THE GATE, beside the restatement and a pinned copy of the same bytes
        best, got = best_of(3, lambda: g.gaf_seqs(memoryview(text)))
        got = np.frombuffer(got, dtype=np.uint8)
        assert got.size == want.size and (got == want).all(), "flatgfa_gaf_seqs differs from the restatement after timing"
        pin_in = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        pin_in.copy_(torch.from_numpy(text))
        pin_out = torch.empty(out_bytes, dtype=torch.uint8, pin_memory=True)
        d_in = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)

        def copies():
            d_in.copy_(pin_in, non_blocking=True)
            pin_out.copy_(d_out, non_blocking=True)
            torch.cuda.synchronize()
        cbest, _ = best_of(3, copies)
        del d_in, d_out, pin_in, pin_out
        torch.cuda.empty_cache()
        res["b_end_to_end"] = {"s": round(best, 4), "gbps_in_plus_out": round((nbytes + out_bytes) / best / 1e9, 2),
                               "cpu_single_thread_s": round(cpu_best, 4), "speedup_vs_cpu": round(cpu_best / best, 2),
                               "gate_faster_than_one_core": bool(best < cpu_best),
                               "pinned_copy_s": round(cbest, 4), "ratio_to_copy": round(best / cbest, 2)}
        del text

        # (c) whole processes
        if not args.skip_cli:
            flat = os.path.join(work, "cfgL.flatgfa")
            g.write_flatgfa(flat)
            t0 = time.perf_counter()
            out_s = subprocess.run([FGFA, "-i", flat, "gaf", gaf, "-s"], capture_output=True, check=True, timeout=900).stdout
            s_s = time.perf_counter() - t0
            assert len(out_s) == out_bytes and (np.frombuffer(out_s, dtype=np.uint8) == want).all(), "fgfa gaf -s differs from the restatement"
            del out_s
            t0 = time.perf_counter()
            out_b = subprocess.run([FGFA, "-i", flat, "gaf", gaf, "-b"], capture_output=True, check=True, timeout=900).stdout
            b_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            cpu_b = subprocess.run(cpu_args + [gaf, "-b"], capture_output=True, check=True, timeout=3000).stdout
            cpu_b_s = time.perf_counter() - t0
            assert out_b == cpu_b, "fgfa gaf -b differs from the restatement"
            res["c_cli"] = {"fgfa_gaf_s_s": round(s_s, 3), "cpu_s_process_s": round(cpu_proc, 3), "fgfa_gaf_b_s": round(b_s, 3),
                            "cpu_b_process_s": round(cpu_b_s, 3), "events": int(out_b)}

        # (d) one long line: a wave walks it alone
        n_tok = 1_000_000
        ids = np.random.default_rng(2).integers(0, len(names), size=n_tok)
        path = b"".join((b">" if i & 1 else b"<") + b"%07d" % int(names[i]) for i in ids)
        total = int(seg_len[ids].sum())
        line = b"long\t1\t0\t1\t+\t" + path + b"\t%d\t%d\t%d\t1\t1\t60\n" % (total, total // 4, total - total // 4)
        lf = os.path.join(work, "long.gaf")
        with open(lf, "wb") as f:
            f.write(line)
        _p, cpu_long = run_cpu(lf, want_file)
        want_long = open(want_file, "rb").read()
        long_s, got_long = best_of(3, lambda: g.gaf_seqs(line))
        assert got_long == want_long, "the long line differs from the restatement"
        res["d_long_line"] = {"line_bytes": len(line), "tokens": n_tok, "out_bytes": len(want_long), "s": round(long_s, 4),
                              "cpu_single_thread_s": round(cpu_long, 4)}
        g.close()
    finally:
        if not args.workdir:
            shutil.rmtree(work, ignore_errors=True)
        else:
            for f in ("reads.gaf", "cfgL.flatgfa", "names.u64", "seq_start.u32", "seq_len.u32", "seq.bin", "gaf_lookup_cpu", "want.txt", "long.gaf"):
                try:
                    os.remove(os.path.join(work, f))
                except OSError:
                    pass
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
