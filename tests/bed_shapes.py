"""BED texts for the intersect tests: the general shapes every route is run on (SHAPES), and the generators the geometry tests
size against the device's layout (csrc/bed_device.hpp, flatten_device.hpp)."""
import random

U64_MAX = (1 << 64) - 1
# the layout the shapes are sized by; tests/test_gpu_bed_geometry.py checks the mirror against the headers
THREADS = 256
CAND_TILE = 1024         # kBedCandTile: candidates a workgroup of the count and fill kernels owns
SCAN_TILE = THREADS * 4  # kBedThreads * kBedScanPer: elements a tile of the three-launch scans
ROUND_CANDS = 1 << 22    # kBedRoundCands
TILE = 16384             # kFlatTile: output bytes a workgroup of the text kernel owns
PIECE = 4 << 20          # kFlatPieceBytes
LONG_NAME = 64           # kFlatLongName


def text(entries) -> bytes:
    return b"".join(b"%s\t%d\t%d\n" % e for e in entries)


def run(name: bytes, n: int, width: int = 10, gap: int = 0, at: int = 0):
    """n sorted, disjoint, non-empty intervals of one name"""
    return [(name, at + i * (width + gap), at + i * (width + gap) + width) for i in range(n)]


def interleave(*groups):
    """the groups' entries line by line in turn"""
    out, k = [], 0
    while any(k < len(g) for g in groups):
        out += [g[k] for g in groups if k < len(g)]
        k += 1
    return out


def flatten_like(name: bytes, n: int) -> bytes:
    """six-column lines under a `#` header, as `fgfa flatten -b` writes them"""
    rows = b"".join(b"%s\t%d\t%d\tp%d\t+\t%d\n" % (name, 7 * i, 7 * i + 7, i % 3, i) for i in range(n))
    return b"#name\tstart\tend\tpath.name\tstrand\tstep.rank\n" + rows


def random_case(rng: random.Random, max_lines: int = 200):
    """at most max_lines x max_lines lines over at most 4 names; sorted and unsorted groups, empty and wrapped-around
    intervals, names only one side has"""
    names = [b"chr1", b"chr2", b"", b"a-much-longer-contig-name"][:rng.randint(1, 4)]
    span = rng.choice([30, 200, 5000])

    def side(n, sort_chance):
        per = {nm: [] for nm in names}
        for _ in range(n):
            s = rng.randrange(span)
            per[rng.choice(names)].append((s, s + rng.randrange(-2, max(3, span // 4))))
        out = []
        for nm in names:
            if rng.random() < sort_chance:
                per[nm].sort(key=lambda iv: iv[0])
            out.append([(nm, s, max(e, 0)) for s, e in per[nm]])
        return interleave(*out) if rng.random() < 0.5 else sum(out, [])
    size = rng.choice([3, 20, 60, max_lines])
    a, b = side(rng.randint(size // 3, size), 0.5), side(rng.randint(size // 3, size), 0.7)
    if len(names) > 1 and rng.random() < 0.3:
        a = [(nm + b"x" if nm == names[-1] else nm, s, e) for nm, s, e in a]  # a name only A has
    return text(a), text(b)


# name -> (a, b): run through every route (whole call, stream, CLI, count, device-level call)
SHAPES = {
    "partial overlap": (b"x\t10\t20\n", b"x\t15\t30\nx\t0\t12\n"),
    "touching": (b"x\t10\t20\n", b"x\t20\t30\nx\t0\t10\n"),
    "nesting": (b"x\t10\t20\nx\t0\t100\n", b"x\t5\t50\nx\t12\t14\n"),
    "duplicates": (b"x\t1\t5\nx\t1\t5\n", b"x\t2\t9\nx\t2\t9\n"),
    "empty name": (b"\t1\t5\nx\t1\t5\n", b"\t2\t9\n"),
    "header and columns": (flatten_like(b"g.og", 12), b"#track\ng.og\t10\t30\tgene\t0\t+\ng.og\t3\t4\nother\t0\t100\n"),
    "unterminated": (b"x\t1\t5\nx\t1\t7", b"x\t0\t9\nx\t0\t3"),
    "u64": (b"x\t5\t18446744073709551615\n", b"x\t0\t18446744073709551615\nx\t18446744073709551614\t18446744073709551615\n"),
    "wrapping numbers": (b"x\t18446744073709551617\t36893488147419103242\n", b"x\t0\t100\n"),
    "interleaved names": (text(interleave(run(b"p", 5, 4, 2), run(b"q", 5, 4, 2, at=3))),
                          text(interleave(run(b"q", 7, 3, 1), run(b"p", 7, 3, 1), run(b"r", 2)))),
    "one side only": (b"onlya\t0\t9\nboth\t0\t9\n", b"onlyb\t0\t9\nboth\t3\t4\n"),
    "empty intervals": (b"x\t5\t5\nx\t9\t2\nx\t0\t50\n", b"x\t7\t7\nx\t30\t3\nx\t1\t2\n"),
    "empty a": (b"", b"x\t1\t2\n"),
    "empty b": (b"x\t1\t2\n", b""),
    "both empty": (b"", b"#nothing\n"),
    "no hit": (b"x\t0\t5\n", b"x\t5\t9\ny\t0\t5\n"),
    "unsorted group": (text(run(b"x", 6, 10, 5) + run(b"y", 3)), text([(b"x", 50, 70), (b"x", 0, 12), (b"x", 20, 95)] + run(b"y", 3))),
    "equal starts": (b"x\t6\t9\n", b"x\t5\t10\nx\t5\t8\nx\t5\t20\n"),
    "nested b": (b"x\t500\t600\n", b"x\t0\t1000\nx\t10\t20\nx\t30\t40\n"),
}
