"""The smallest sequence pools at which each seam of the crush kernels (pollen_amd/csrc/crush_device.hip) can break: tiles of
T laid-out bytes, waves of 64, 16-byte output vectors, the segment scans' tiles and spine, and the ranges of tiles a
workgroup walks.  SHAPES maps a name to a function that makes the pools; tests/test_crush_model.py holds the model's two
forms to each other on every shape and checks what the names say, tests/test_gpu_crush_geometry.py runs them on the device."""
from __future__ import annotations

from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

import crush_model as cm
from oracle import flatgfa_oracle as fo

T = cm.TILE


def pools(seq_data, spans: Sequence[Tuple[int, int]]) -> fo.Pools:
    """Pools with these segment spans (start, end) into seq_data, named 1.., and nothing else."""
    seq = np.frombuffer(bytes(seq_data), np.uint8).copy() if not isinstance(seq_data, np.ndarray) else seq_data
    segs = np.zeros(len(spans), fo.SEG_DT)
    if len(spans):
        a = np.array(spans, dtype=np.int64).reshape(-1, 2)
        segs["name"], segs["seq_start"], segs["seq_end"] = np.arange(1, len(spans) + 1), a[:, 0], a[:, 1]
    z = np.zeros(0, np.uint8)
    return fo.Pools(header=z, segs=segs, paths=np.zeros(0, fo.PATH_DT), links=np.zeros(0, fo.LINK_DT), steps=np.zeros(0, np.uint32),
                    seq_data=seq, overlaps=np.zeros(0, fo.SPAN_DT), alignment=np.zeros(0, np.uint32), name_data=z, optional_data=z,
                    line_order=z)


def of_seqs(seqs: List[bytes]) -> fo.Pools:
    """The segments one behind another."""
    spans, at = [], 0
    for s in seqs:
        spans.append((at, at + len(s)))
        at += len(s)
    return pools(b"".join(seqs), spans)


def filler(n: int, seed: int = 0) -> bytes:
    """n bytes of ACGT, no N."""
    return bytes(b"ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))


def run_with_first_drop_at(d: int) -> fo.Pools:
    # one segment: N at d - 1 is kept, d .. d + 4 are dropped
    return of_seqs([filler(d - 1) + b"N" * 6 + filler(T, 1)])


def seam_at(q: int) -> fo.Pools:
    # a seam at laid-out offset q with N on both sides: both are kept
    return of_seqs([filler(q - 1) + b"N", b"N" + filler(40, 2)])


def ending_at(k: int) -> fo.Pools:
    # no N: the kept bytes end k bytes past a 16-byte boundary; with one run early on, so that the tile's bytes move
    return of_seqs([filler(100, 3) + b"NNN" + filler(4096 + k - 101, 4)])


def many(n: int) -> fo.Pools:
    # n segments of one to three bytes, every fifth an N, every seventh NN; two empty ones
    rng = np.random.default_rng(n)
    i = np.arange(n)
    lens = rng.integers(1, 4, n)
    lens[i % 5 == 0] = 1
    lens[i % 7 == 0] = 2
    lens[[n // 3, n - 1]] = 0
    end = np.cumsum(lens)
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(end[-1]))].copy()
    pool[np.repeat((i % 5 == 0) | (i % 7 == 0), lens)] = cm.N
    return pools(pool, np.stack([end - lens, end], axis=1))


def aliased() -> fo.Pools:
    pool = filler(50, 5) + b"NNNN" + filler(30, 6) + b"NN" + filler(16, 7)
    n = len(pool)
    # out of order, overlapping, two that share one range (two copies in the output), one inside a run, one ending at seq_len
    return pools(pool, [(60, n), (0, 58), (48, 56), (48, 56), (51, 53), (10, 10), (0, n), (n, n)])


def tiles_past_the_grid() -> fo.Pools:
    # more tiles than workgroups, so that a workgroup walks two tiles: 1 MiB of pool with runs, aliased 33 times over
    rng = np.random.default_rng(9)
    pool = rng.choice(np.frombuffer(b"ACGTN", np.uint8), 1 << 20, p=[0.2, 0.2, 0.2, 0.2, 0.2])
    spans = [(0, 1 << 20)] * 32 + [(5, (1 << 20) - 3), (7, 7), (100, 100 + T + 9)]
    return pools(pool, spans)


SHAPES: Dict[str, Callable[[], fo.Pools]] = {
    "first drop at T-1": lambda: run_with_first_drop_at(T - 1),
    "first drop at T": lambda: run_with_first_drop_at(T),
    "first drop at T+1": lambda: run_with_first_drop_at(T + 1),
    "run ends at T": lambda: of_seqs([filler(T - 5) + b"N" * 5 + filler(70, 1)]),
    "seam at T, N on both sides": lambda: seam_at(T),
    "seam at T-1, N on both sides": lambda: seam_at(T - 1),
    "seam at T+1, N on both sides": lambda: seam_at(T + 1),
    "3T+5 of N": lambda: of_seqs([b"N" * (3 * T + 5)]),
    "3T+5 of N, then NA": lambda: of_seqs([b"N" * (3 * T + 5), b"NA"]),
    "empty segment first": lambda: of_seqs([b"", b"NNA", b"C"]),
    "empty segment last": lambda: of_seqs([b"ANN", b"C", b""]),
    "empty segments at a tile edge": lambda: of_seqs([filler(T - 1) + b"N", b"", b"", b"", b"NNC", b"", filler(T), b"", b""]),
    "only empty segments": lambda: of_seqs([b""] * 5),
    "no segments": lambda: of_seqs([]),
    "no segments, a pool": lambda: pools(b"NNNN", []),
    "single N segments over a tile": lambda: pools(b"NN", [(i & 1, (i & 1) + 1) for i in range(T + 100)]),
    "kept bytes end at 16k+15": lambda: ending_at(15),
    "kept bytes end at 16k+16": lambda: ending_at(16),
    "kept bytes end at 16k+17": lambda: ending_at(17),
    "a wave of one segment each": lambda: of_seqs([b"N"] * 64 + [b"NN"] * 64 + [b"NNN"] * 64),
    "scan tile - 1 segments": lambda: many(cm.SCAN_TILE - 1),
    "scan tile segments": lambda: many(cm.SCAN_TILE),
    "scan tile + 1 segments": lambda: many(cm.SCAN_TILE + 1),
    "spine's second round": lambda: many(cm.THREADS * cm.SCAN_TILE + 1),
    "out of order, overlapping, aliased": aliased,
    "more tiles than workgroups": tiles_past_the_grid,
}
