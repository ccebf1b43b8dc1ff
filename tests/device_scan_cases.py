"""Cases for tests/device_check/scan_check.hip, the stand-alone program over pollen_amd/csrc/device_scan.hpp: what goes into
each case's input file, how its output file is laid out, and what the output must be, from Python integers and numpy.  The
layouts restate the table at the head of scan_check.hip.  tests/test_gpu_device_scan.py runs the cases on the GPU;
tests/test_device_scan_cases.py checks the generators and the references themselves on the CPU.

A case makes its input afresh from its seed each time it is asked (the large ones are tens of megabytes): nothing is kept.

The references:
  sum32, sum64   the exclusive prefix in Python integers / numpy's wrapping integers, mod 2^32 or 2^64; the total of sum32 is
                 exact (the spine is 64 bits wide), that of sum64 is mod 2^64.
  affine         x -> a x + b mod 2^64, composed from the left.  affine_reference() does it one element at a time in Python
                 integers.  That takes seconds for millions of elements, so check_affine() verifies the same definition a step
                 at a time instead, on numpy's wrapping u64: out[0] is the identity, out[i + 1] = out[i] then in[i], the total is
                 out[n - 1] then in[n - 1].  By induction that is the sequential composition and nothing else; up to
                 AFFINE_BY_HAND elements both are done, and the CPU tests pin one to the other.
"""
import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
GUARD_BYTE = 0xA5
POINTS = ((256, 4), (256, 8), (64, 1), (1024, 2))  # (kThreads, kPer) of the tiled scans
BLOCK_THREADS = (64, 256, 1024)
WAVE_THREADS = 256
SMALL_GUARD = 256       # guard elements of last_start and check_links
MAX_N = 1 << 23         # what the program takes for n
AFFINE_BY_HAND = 70_000


def tile(point):
    return point[0] * point[1]


def point_name(point):
    return "%dx%d" % point


def sizes(point):
    """The lengths the issue names: round the lanes' items, a tile, and a round of the spine (kThreads tiles)."""
    kt, kp = point
    t = kt * kp
    out = []
    for n in (0, 1, kp - 1, kp, t - 1, t, t + 1, 2 * t + 3, kt * t - 1, kt * t, kt * t + 1, 2 * kt * t + 1):
        if n not in out:
            out.append(n)
    return out


class Case:
    """kind, point (the manifest's word), n, name; make_input() -> bytes; check(out_bytes) asserts."""

    def __init__(self, kind, point, n, name, make, check):
        self.kind, self.point, self.n, self.name, self._make, self._check = kind, point, n, name, make, check

    @property
    def id(self):
        return "%s-%s-n%d%s" % (self.kind, self.point, self.n, "-" + self.name if self.name else "")

    def arrays(self):
        return self._make()

    def make_input(self):
        a = self._make()
        return b"".join(np.ascontiguousarray(x).tobytes() for x in (a if isinstance(a, tuple) else (a,)))

    def check(self, out: bytes):
        self._check(self._make(), out)


def split_guard(out: bytes, dtype, count, guard, what):
    """The first `count` elements of a guarded array at the head of `out`, and the bytes behind array and guard."""
    item = np.dtype(dtype).itemsize
    assert len(out) >= (count + guard) * item, "%s: output of %d bytes is short of %d elements" % (what, len(out), count + guard)
    body = np.frombuffer(out, dtype, count)
    g = np.frombuffer(out, np.uint8, guard * item, count * item)
    bad = np.flatnonzero(g != GUARD_BYTE)
    assert not len(bad), "%s: the guard behind element %d was written at byte %d" % (what, count, int(bad[0]))
    return body, out[(count + guard) * item:]


# ---- sum32 ----

def sum32_spiky(n, seed):
    """Values below 2^20 and one of 2^31 every 4096 elements: any 2048 consecutive ones sum to less than 2^32."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    if n:
        a[int(rng.integers(0, min(n, 4096)))::4096] = 1 << 31
    return a


def sum32_big(n, seed):
    """2^22 on every fourth element (at most 512 of them in a tile: 2^31), values below 2^12 between them: past 4 096
    elements the total is above 2^32 while no tile's sum is."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 12, n, dtype=np.uint32)
    a[::4] = 1 << 22
    return a


def sum32_reference(a):
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)   # (below 2^23 elements of less than 2^32: no wrap in 64 bits)
    excl = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if len(a) else c
    return (excl & np.uint64(M32)).astype(np.uint32), int(c[-1]) if len(a) else 0


def check_sum32(point, a, out):
    n = len(a)
    got, rest = split_guard(out, np.uint32, n, tile(point), "sum32")
    assert len(rest) == 8
    want, total = sum32_reference(a)
    bad = np.flatnonzero(got != want)
    assert not len(bad), "first wrong prefix at element %d: %d, not %d" % (bad[0], got[bad[0]], want[bad[0]])
    assert int(np.frombuffer(rest, np.uint64)[0]) == total, "total %d, not %d" % (int(np.frombuffer(rest, np.uint64)[0]), total)


# ---- sum64 ----

def sum64_input(point, n, seed):
    """Random 40-bit values and a few of 2^63: at both ends, in the middle and on either side of the first tile edge."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    t = tile(point)
    for i in (0, n // 2, t - 1, t, n - 1):
        if 0 <= i < n:
            a[i] = 1 << 63
    return a


def check_sum64(point, a, out):
    n = len(a)
    got, rest = split_guard(out, np.uint64, n, tile(point), "sum64")
    assert len(rest) == 8
    c = np.cumsum(a, dtype=np.uint64)  # (wraps mod 2^64)
    want = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if n else c
    bad = np.flatnonzero(got != want)
    assert not len(bad), "first wrong prefix at element %d: %d, not %d" % (bad[0], got[bad[0]], want[bad[0]])
    total, wtotal = int(np.frombuffer(rest, np.uint64)[0]), int(c[-1]) if n else 0
    assert total == wtotal, "total %d, not %d" % (total, wtotal)


# ---- affine ----

def affine_input(n, seed):
    rng = np.random.default_rng(seed)
    ab = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    ab[:, 0] |= np.uint64(1)
    return ab


def affine_reference(ab):
    """The carries in front of every element, and the total: sequential composition in Python integers."""
    a, b = 1, 0
    out = []
    for ya, yb in ab.tolist():
        out.append((a, b))
        a, b = (ya * a) & M64, (ya * b + yb) & M64
    return out, (a, b)


def affine_then(x, y):
    """x, then y, elementwise on u64 pairs (rows)."""
    with np.errstate(over="ignore"):
        return np.stack([y[:, 0] * x[:, 0], y[:, 0] * x[:, 1] + y[:, 1]], axis=1)


def affine_step_errors(ab, got, total):
    """Indices i at which got[i] is not what the definition makes of got[i - 1] and ab[i - 1]; n stands for the total."""
    n = len(ab)
    if not n:
        return [] if tuple(int(x) for x in total) == (1, 0) else [0]
    want = np.concatenate([np.array([[1, 0]], np.uint64), affine_then(got, ab)])  # want[i + 1] from got[i]
    have = np.concatenate([got, np.asarray(total, np.uint64).reshape(1, 2)])
    return [int(i) for i in np.flatnonzero((want != have).any(axis=1))]


def check_affine(point, ab, out):
    n = len(ab)
    got, rest = split_guard(out, np.uint64, 2 * n, 2 * tile(point), "affine")
    assert len(rest) == 16
    got = got.reshape(n, 2)
    total = np.frombuffer(rest, np.uint64)
    bad = affine_step_errors(ab, got, total)
    assert not bad, "first wrong carry at element %d of %d (n: the total)" % (bad[0], n)
    if n <= AFFINE_BY_HAND:
        want, wtotal = affine_reference(ab)
        assert [tuple(r) for r in got.tolist()] == want and tuple(total.tolist()) == wtotal


# ---- block_excl ----

def block_values(bits, threads, name, seed):
    """Two calls' lane values.  `bits`: random over the full width with bit 31 (and bit 63) forced on some lanes; `ones`: every
    bit of every lane; `lone`: zeros but for bit 31 / bit 63 on single lanes at the waves' edges."""
    rng = np.random.default_rng(seed)
    dt = np.uint32 if bits == 32 else np.uint64
    if name == "ones":
        v = np.full(2 * threads, (1 << bits) - 1, dt)
        v[threads:] -= np.arange(threads, dtype=dt)
    elif name == "lone":
        v = np.zeros(2 * threads, dt)
        for k, i in enumerate((0, 31, 32, 63, threads - 64, threads - 1)):
            v[i] |= dt(1 << (31 if k % 2 == 0 or bits == 32 else 63))
            v[threads + i] |= dt(1 << (bits - 1))
    else:
        v = rng.integers(0, 1 << bits, 2 * threads, dtype=dt)
        v[rng.random(2 * threads) < 0.3] |= dt(1 << 31)
        if bits == 64:
            v[rng.random(2 * threads) < 0.3] |= dt(1 << 63)
            v[rng.random(2 * threads) < 0.1] &= dt(M32 << 32)  # (an empty low half under a full high one)
    return v


def check_block_excl(bits, threads, v, out):
    dt = np.uint32 if bits == 32 else np.uint64
    got, rest = split_guard(out, dt, 4 * threads, threads, "block_excl")
    assert not rest
    mask = (1 << bits) - 1
    for call in range(2):
        vals = [int(x) for x in v[call * threads:(call + 1) * threads]]
        run, want = 0, []
        for x in vals:
            want.append(run)
            run = (run + x) & mask
        res = got[call * threads:(call + 1) * threads].tolist()
        tot = got[(2 + call) * threads:(3 + call) * threads].tolist()
        assert res == want, "call %d: first wrong lane %d" % (call + 1, next(i for i in range(threads) if res[i] != want[i]))
        assert tot == [run] * threads, "call %d: total" % (call + 1)


# ---- wave ----

def wave_values(name, seed):
    """256 values (the classes of block_values, 64 bits wide) and each lane's source lane: a permutation of every wave."""
    rng = np.random.default_rng(seed)
    v = block_values(64, WAVE_THREADS // 2, name, seed)
    src = np.concatenate([rng.permutation(64) for _ in range(WAVE_THREADS // 64)]).astype(np.uint64)
    return v, src


def check_wave(arrays, out):
    v, src = arrays
    n = WAVE_THREADS
    got, rest = split_guard(out, np.uint64, 5 * n, n, "wave")
    assert not rest
    got = got.reshape(5, n).tolist()
    vals = [int(x) for x in v]
    for w in range(n // 64):
        lanes = vals[w * 64:(w + 1) * 64]
        incl, run = [], 0
        for x in lanes:
            run = (run + x) & M64
            incl.append(run)
        sl = slice(w * 64, (w + 1) * 64)
        assert got[0][sl] == [run] * 64, "wave_sum, wave %d" % w
        assert got[1][sl] == incl, "wave_incl_scan, wave %d" % w
        assert got[2][sl] == [lanes[0]] * 64, "shfl_u64 from lane 0, wave %d" % w
        assert got[3][sl] == [lanes[63]] * 64, "shfl_u64 from lane 63, wave %d" % w
        assert got[4][sl] == [lanes[int(s)] for s in src[sl]], "shfl_u64 from a lane of its own, wave %d" % w


# ---- last_start ----

def last_start_table(name):
    """(pstart, lo, hi, queries).  Queries are at or past pstart[lo]: in front of it no path of [lo, hi] holds the step."""
    rng = np.random.default_rng(7)
    if name == "top":  # starts up to 2^32 - 1, the last ones equal
        ps = np.array([0, 5, 5, 1 << 31, M32 - 1, M32, M32], np.uint64)
        lo, hi = 0, len(ps) - 1
        q = [0, 4, 5, 6, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, M32 - 2, M32 - 1, M32, 1 << 32, 1 << 40, M64]
    else:
        steps = rng.integers(0, 4, 999)
        steps[rng.random(999) < 0.3] = 0          # runs of equal starts: empty paths
        steps[100:110] = 0
        ps = np.concatenate([[0], np.cumsum(steps)]).astype(np.uint64)
        lo, hi = {"whole": (0, 999), "inner": (3, 700), "one": (5, 5), "first": (0, 0), "pair": (998, 999)}[name]
        inside = [int(x) for x in ps[lo:hi + 1]]
        q = inside + [x - 1 for x in inside if x > inside[0]] + [x + 1 for x in inside] + [int(ps[-1]) + 9, 1 << 33]
        q += list(rng.integers(int(ps[lo]), int(ps[-1]) + 2, 300))
    return ps, lo, hi, np.array([int(x) for x in q], np.uint64)


def last_start_arrays(name):
    ps, lo, hi, q = last_start_table(name)
    return np.array([len(ps), lo, hi], np.uint64), ps, q


def check_last_start(arrays, out):
    (m, lo, hi), ps, q = arrays
    lo, hi = int(lo), int(hi)
    got, rest = split_guard(out, np.uint32, len(q), SMALL_GUARD, "last_start")
    assert not rest
    want = np.searchsorted(ps[lo:hi + 1], q, side="right") - 1 + lo
    assert (want >= lo).all()
    bad = np.flatnonzero(got != want)
    assert not len(bad), "step %d: path %d, not %d" % (int(q[bad[0]]), got[bad[0]], want[bad[0]])


# ---- check_links ----

LINKS_N, LINKS_SEGS, LINKS_BEFORE = 1000, 50, 8


def links_arrays(bad_at, end, bit):
    """A table of LINKS_N links over LINKS_SEGS segments, the last segment named in both orientations, with spans that
    are no segment ids; bad_at (None: clean) gets LINKS_SEGS as its `end` (0: from, 1: to)."""
    rng = np.random.default_rng(11)
    lk = np.zeros((LINKS_N, 4), np.uint32)
    lk[:, :2] = (rng.integers(0, LINKS_SEGS, (LINKS_N, 2)) << 1) | rng.integers(0, 2, (LINKS_N, 2))
    lk[::7, 0] = ((LINKS_SEGS - 1) << 1) | 1
    lk[3::7, 1] = ((LINKS_SEGS - 1) << 1) | 1
    lk[:, 2:] = rng.integers(1 << 20, 1 << 32, (LINKS_N, 2))
    if bad_at is not None:
        lk[bad_at, end] = LINKS_SEGS << 1
    return np.array([LINKS_SEGS, bit, LINKS_BEFORE], np.uint32), lk


def check_check_links(bad, arrays, out):
    got, rest = split_guard(out, np.uint32, 1, SMALL_GUARD, "check_links")
    assert not rest
    bit = int(arrays[0][1])
    assert int(got[0]) == (LINKS_BEFORE | bit if bad else LINKS_BEFORE), "flags %#x" % int(got[0])


# ---- blocks ----

def blocks_arrays():
    rows = []
    for per in (1, 256, 1024):
        for grid in (1, 2048):
            rows += [(n, per, grid) for n in (0, 1, per, per + 1, per * grid - 1, per * grid, per * grid + 1, per * (grid + 1), 1 << 40)]
    rows.append((M32 * 1024, 1024, M32))
    rows.append((M32 * 1024 + 1, 1024, M32))
    return np.array(rows, np.uint64)


def check_blocks(rows, out):
    got = np.frombuffer(out, np.uint64).reshape(-1, 2).tolist()
    want = []
    for n, per, grid in rows.tolist():
        b = -(-n // per)
        want.append([b, min(max(b, 1), grid)])
    assert got == want


# ---- the manifest ----

def tiled_cases():
    out = []
    for point in POINTS:
        pn = point_name(point)
        big_from = point[0] * tile(point) - 1
        for n in sizes(point):
            s = [point[0], point[1], n]
            out.append(Case("sum32", pn, n, "spiky", lambda n=n, s=s: sum32_spiky(n, s + [1]), lambda a, o, p=point: check_sum32(p, a, o)))
            if n >= big_from:
                out.append(Case("sum32", pn, n, "big", lambda n=n, s=s: sum32_big(n, s + [2]), lambda a, o, p=point: check_sum32(p, a, o)))
            out.append(Case("sum64", pn, n, "", lambda n=n, s=s, p=point: sum64_input(p, n, s + [3]), lambda a, o, p=point: check_sum64(p, a, o)))
            out.append(Case("affine", pn, n, "", lambda n=n, s=s: affine_input(n, s + [4]), lambda a, o, p=point: check_affine(p, a, o)))
    return out


def small_cases():
    out = []
    for bits in (32, 64):
        for threads in BLOCK_THREADS:
            for name in ("bits", "ones", "lone"):
                out.append(Case("block_excl", "u%dx%d" % (bits, threads), threads, name,
                                lambda b=bits, t=threads, nm=name: block_values(b, t, nm, [b, t, 5]),
                                lambda v, o, b=bits, t=threads: check_block_excl(b, t, v, o)))
    for name in ("bits", "ones", "lone"):
        out.append(Case("wave", "-", WAVE_THREADS, name, lambda nm=name: wave_values(nm, [6]), check_wave))
    for name in ("whole", "inner", "one", "first", "pair", "top"):
        out.append(Case("last_start", "-", len(last_start_table(name)[3]), name, lambda nm=name: last_start_arrays(nm), check_last_start))
    for at in (0, 255, 256, LINKS_N - 1):
        for end, bit in ((0, 2), (1, 4)):
            out.append(Case("check_links", "-", LINKS_N, "%s%d-bit%d" % ("from" if end == 0 else "to", at, bit),
                            lambda at=at, end=end, bit=bit: links_arrays(at, end, bit), lambda a, o: check_check_links(True, a, o)))
    out.append(Case("check_links", "-", LINKS_N, "clean", lambda: links_arrays(None, 0, 2), lambda a, o: check_check_links(False, a, o)))
    out.append(Case("blocks", "-", len(blocks_arrays()), "", blocks_arrays, check_blocks))
    return out


CASES = tiled_cases() + small_cases()
