"""The pangenotype matrix at scale: one JSON line.

    python tools/pangenotype_bench.py [--gb 4] [--workdir DIR] [--out FILE] [--skip-cli]

A seeded GAF of --gb gigabytes over the cfg-L graph (bench.py's cfgL: synth(1, 1 M segments, 1000 paths of 100 k steps)):
short-read-like lines -- a read name, query columns, a path field of 5-20 nodes (`>`/`<`, names zero-padded to seven digits;
the count is drawn per block of 65536 lines), target columns and NM/AS/dv/id/cg tags.  The bits are checked against the
generator's own record of the names it wrote before anything is timed.  Then:

  (a) kernel_gbps      flatgfa_dev_pangenotype_row on device-resident text (64 MB, 512 MB, 2 GB), HIP events, warm, best of 5
  (b) e2e_gbps         host buffer -> bits (FlatGFA.pangenotype_matrix on text in anonymous memory), beside a plain H2D copy
                       of the same bytes from pinned memory in the same process; best of 3 each
  (c) cli_s            `fgfa -i cfgL.flatgfa matrix GAF`, whole process, beside the single-thread C++ restatement of
                       pangenotype.rs (tools/pangenotype_cpu.cpp, compiled here with g++ -O3); their outputs must agree.
                       Both read the GAF from the page cache (it was just written and read).

The GAF is written under --workdir (default: a temporary directory) and removed at the end.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pollen_amd as pa  # noqa: E402
from pollen_amd import device as pdev  # noqa: E402

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
BLOCK = 65536
DIGITS = 7


def gaf_block(rng, names, first_read, n_tok):
    """BLOCK lines of n_tok nodes each, as a (BLOCK, width) uint8 array, and the segment ids they name."""
    head = b"r%010d\t150\t0\t150\t+\t"
    tail = np.frombuffer(b"\t5000\t1200\t1350\t148\t150\t60\tNM:i:2\tAS:f:140\tdv:f:0.013\tid:f:0.987\tcg:Z:150M\n", dtype=np.uint8)
    hw = len(head % 0)
    width = hw + n_tok * (DIGITS + 1) + len(tail)
    a = np.empty((BLOCK, width), dtype=np.uint8)
    rid = np.arange(first_read, first_read + BLOCK, dtype=np.int64)
    a[:, :hw] = np.frombuffer(head % 0, dtype=np.uint8)
    for d in range(10):  # the read number's ten digits
        a[:, 10 - d] = (rid // 10 ** d % 10).astype(np.uint8) + ord("0")
    a[:, -len(tail):] = tail
    ids = rng.integers(0, len(names), size=(BLOCK, n_tok), dtype=np.int64)
    tok = a[:, hw:hw + n_tok * (DIGITS + 1)].reshape(BLOCK, n_tok, DIGITS + 1)
    tok[:, :, 0] = np.where(rng.random((BLOCK, n_tok)) < 0.5, ord(">"), ord("<"))
    v = names[ids]
    for d in range(DIGITS, 0, -1):
        tok[:, :, d] = (v % 10).astype(np.uint8) + ord("0")
        v = v // 10
    return a, ids


def write_gaf(path, names, gb, seed=1):
    rng = np.random.default_rng(seed)
    want = np.zeros(len(names), dtype=bool)
    total, reads = 0, 0
    with open(path, "wb") as f:
        while total < gb * (1 << 30):
            a, ids = gaf_block(rng, names, reads, int(rng.integers(5, 21)))
            f.write(a.tobytes())
            want[ids.ravel()] = True
            total += a.size
            reads += BLOCK
    return total, want


def cut(text, n):
    """The first n bytes of text, cut back to just after a newline."""
    return int(np.flatnonzero(text[:n] == 10)[-1]) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4.0)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    args = ap.parse_args()
    import torch
    work = args.workdir or tempfile.mkdtemp(prefix="pangenotype_bench_")
    os.makedirs(work, exist_ok=True)
    res = {"what": "pangenotype matrix (fgfa matrix) over cfg-L", "graph": "synth(1, 1000000, 1000, 100000, pangenome)"}
    try:
        t = time.perf_counter()
        g = pa.synth(1, 1_000_000, 1000, 100_000, "pangenome", False)
        names = np.asarray(g.pool("segs")["name"], dtype=np.uint64)
        assert names.max() < 10 ** DIGITS
        S = len(names)
        gaf = os.path.join(work, "reads.gaf")
        nbytes, want = write_gaf(gaf, names, args.gb)
        res.update(gaf_bytes=nbytes, segments=S, covered=int(want.sum()), generate_s=round(time.perf_counter() - t, 1))
        text = np.fromfile(gaf, dtype=np.uint8)  # anonymous memory, not the mapping

        # check first: the library's bits against the generator's record
        got = g.pangenotype_matrix([memoryview(text)])[0]
        assert (got == want).all(), "bits differ from the generator"
        res["bits_match_generator"] = True

        # (a) kernel only, device-resident text
        dev = torch.device("cuda:0")
        W = (S + 63) // 64
        row = torch.zeros(W, dtype=torch.int64, device=dev)
        bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
        kern = {}
        for size in (64 << 20, 512 << 20, 2 << 30):
            if size > nbytes:
                continue
            n = cut(text, size)
            d = torch.from_numpy(text[:n]).to(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            best = 1e9
            for rep in range(6):
                ev[0].record()
                pdev.pangenotype_row(g, d, row, bad)
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    best = min(best, ev[0].elapsed_time(ev[1]))
            assert int(bad.item()) == -1
            kern[f"{n >> 20}MB"] = {"ms": round(best, 3), "gbps": round(n / best / 1e6, 1)}
            del d
        bits = np.unpackbits(row.cpu().numpy().view(np.uint8), bitorder="little")[:S].astype(bool)
        assert not (bits & ~want).any()
        res["a_kernel"] = kern
        torch.cuda.empty_cache()

        # (b) host buffer -> bits, beside a pinned H2D copy of the same bytes
        best = 1e9
        for _ in range(3):
            t = time.perf_counter()
            got = g.pangenotype_matrix([memoryview(text)])
            best = min(best, time.perf_counter() - t)
        assert (got[0] == want).all()
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        pinned.copy_(torch.from_numpy(text))
        d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cbest = 1e9
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            cbest = min(cbest, time.perf_counter() - t)
        del d, pinned
        torch.cuda.empty_cache()
        res["b_end_to_end"] = {"s": round(best, 4), "gbps": round(nbytes / best / 1e9, 2), "pinned_h2d_s": round(cbest, 4),
                               "pinned_h2d_gbps": round(nbytes / cbest / 1e9, 2), "ratio_to_copy": round(best / cbest, 3)}
        del text

        # (c) whole processes: fgfa matrix against the single-thread restatement
        if not args.skip_cli:
            flat = os.path.join(work, "cfgL.flatgfa")
            g.write_flatgfa(flat)
            nm = os.path.join(work, "names.u64")
            names.astype("<u8").tofile(nm)
            cpu = os.path.join(work, "pangenotype_cpu")
            subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", os.path.join(ROOT, "tools", "pangenotype_cpu.cpp"), "-o", cpu])
            t = time.perf_counter()
            out_gpu = subprocess.run([FGFA, "-i", flat, "matrix", gaf], capture_output=True, check=True, timeout=600).stdout
            gpu_s = time.perf_counter() - t
            t = time.perf_counter()
            out_cpu = subprocess.run([cpu, nm, gaf], capture_output=True, check=True, timeout=1800).stdout
            cpu_s = time.perf_counter() - t
            assert out_gpu == out_cpu, "fgfa matrix differs from the single-thread restatement"
            res["c_cli"] = {"fgfa_matrix_s": round(gpu_s, 3), "cpu_single_thread_s": round(cpu_s, 3), "speedup": round(cpu_s / gpu_s, 1)}
        g.close()
    finally:
        if not args.workdir:
            shutil.rmtree(work, ignore_errors=True)
        else:
            for f in ("reads.gaf", "cfgL.flatgfa", "names.u64", "pangenotype_cpu"):
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
