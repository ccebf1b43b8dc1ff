"""The build of the sorted record image (pollen_amd/csrc/depth_sorted.hip: sorted_image_count, sorted_image_emit,
sorted_image_finalise; DESIGN.md sections 3.2, 3.3) on its own: the cases tests/device_check/sorted_image_check.hip runs, a model
of what the build must leave, and the checker that holds a dumped image to the model.

A case is what the build reads of a plan: items (the steps [b, e) of a path or of a piece of one, and the path's id), the run
image's entries (a run of consecutive segment ids going up or down by one, and the step it begins at), the stretch of entries
each item reads, and wb, n_range, n_win, n_paths, n_cus.  `Builder` lays runs into a step array and cuts items out of it; it
asserts what the build takes for granted and nothing tests: a run has at most 1024 steps, an item's entries cover its steps,
the entries' positions ascend.

The model is written from the design, not from the kernels: it expands the entries into the id of every step, takes an item's
part of each entry as a stretch of ids, and cuts that at the window edges.  A record is (window, path, window-relative start,
length - 1); a window's records are ordered by path, then start; the first of each path is flagged, a record carries the number
of flags in its chunk of 64 up to itself, a window is padded to whole chunks, and a chunk's carry is the largest end among the
earlier records, in the window, of the path the chunk begins inside (0 where it begins a path).  The order of records with the
same window, path and start is the sort's (emission goes through an atomic cursor), so the checker compares multisets per path
and recomputes ordinals and carries from the order it finds.  tests/test_sorted_image_cases.py ties the model to brute force on
the CPU; tests/test_gpu_sorted_image.py runs the program.
"""
import collections
import struct

import numpy as np

CHUNK = 64
FIRST = 1 << 23
PAD = 1 << 31
ORD_SHIFT = 24
ORD_MASK = 0x7F
MAX_RUN = 1024
HIST_WINDOWS = 8192  # the count kernel's LDS histogram holds this many windows; beyond, it counts straight into memory

Run = collections.namedtuple("Run", "first n dn")


def R(first, n, dn=False):
    """A run of n steps from id `first`, going up by one (dn: down by one)."""
    return Run(first, n, dn)


def shorts(n, base, stride=3, length=2):
    assert stride > length
    return [R(base + stride * i, length) for i in range(n)]


class Builder:
    """Runs laid one behind the other into a step array, and items cut out of it."""

    def __init__(self):
        self.ent = []      # (first, dn, position)
        self.n_steps = 0
        self.items = []    # (b, e, path, ent_lo, ent_hi)

    def lay(self, runs):
        """Appends the runs; returns (index of the first entry, of the one behind the last, first step, step behind the last)."""
        lo, b = len(self.ent), self.n_steps
        for r in runs:
            assert 1 <= r.n <= MAX_RUN, "a run has at most 1024 steps"
            self.ent.append((r.first, r.dn, self.n_steps))
            self.n_steps += r.n
        return lo, len(self.ent), b, self.n_steps

    def item(self, path, b, e, slack=(0, 0), ent=None):
        """An item over the steps [b, e): it reads the entries its steps lie in and `slack` more on either side."""
        assert b < e <= self.n_steps
        pos = [p for _, _, p in self.ent]
        if ent is None:
            lo = max(i for i, p in enumerate(pos) if p <= b)
            hi = max(i for i, p in enumerate(pos) if p < e) + 1
            ent = (max(lo - slack[0], 0), min(hi + slack[1], len(self.ent)))
        self.items.append((b, e, path, ent[0], ent[1]))

    def path(self, path, runs, slack=(0, 0)):
        """One item over exactly these runs."""
        _, _, b, e = self.lay(runs)
        self.item(path, b, e, slack)

    def pieces(self, path, runs, cuts, slack=(0, 0)):
        """The runs as one path cut into items at (run, steps into it) -- a piece may begin and end inside a run."""
        lo, _, b, e = self.lay(runs)
        at = [b] + [self.ent[lo + k][2] + off for k, off in cuts] + [e]
        assert all(x < y for x, y in zip(at, at[1:]))
        for x, y in zip(at, at[1:]):
            self.item(path, x, y, slack)


class Case:
    def __init__(self, id, wb, n_range, n_paths, build, n_cus=1, n_win=None, reserve=0, waived=False, second=None, verdict="built", prop=None,
                 unchecked=False):
        self.id, self.wb, self.n_range, self.n_paths, self.n_cus = id, wb, n_range, n_paths, n_cus
        self.n_win = n_win if n_win is not None else (n_range + (1 << wb) - 1) >> wb
        self.reserve, self.waived, self.verdict, self.prop = reserve, waived, verdict, prop
        b = Builder()
        build(b)
        self.items = np.array([(x, y, 0, p) for x, y, p, _, _ in b.items], dtype=np.uint32).reshape(-1, 4)
        self.item_ent = np.array([(lo, hi) for _, _, _, lo, hi in b.items], dtype=np.uint32).reshape(-1, 2)
        self.ent = self.entries_of(b.ent, b.n_steps)
        self.ent2 = None
        if second is not None:
            b2 = Builder()
            second(b2)
            self.ent2 = self.entries_of(b2.ent, b2.n_steps)
            assert self.ent2.shape == self.ent.shape and (self.ent2[:, 1] == self.ent[:, 1]).all(), "the second array has the first one's positions"
        if not unchecked:
            self.assert_preconditions()

    @staticmethod
    def entries_of(ent, n_steps):
        rows = [(first | (1 << 31 if dn else 0), pos) for first, dn, pos in ent] + [(0, n_steps)]
        return np.array(rows, dtype=np.uint32).reshape(-1, 2)

    def assert_preconditions(self):
        """What the build takes for granted: not tested, so every case must meet it."""
        pos = self.ent[:, 1].astype(np.int64)
        assert (np.diff(pos) > 0).all() and (np.diff(pos) <= MAX_RUN).all(), self.id
        assert self.n_win == (self.n_range + (1 << self.wb) - 1) >> self.wb, self.id
        for (b, e, _, path), (lo, hi) in zip(self.items.tolist(), self.item_ent.tolist()):
            assert path < self.n_paths, self.id
            assert lo < hi <= len(self.ent) - 1 and pos[lo] <= b < e <= pos[hi], (self.id, "an item's entries cover its steps")

    def make_input(self):
        head = struct.pack("<10Q", self.wb, self.n_range, self.n_win, self.n_paths, self.n_cus, self.reserve, int(self.waived), len(self.items),
                           len(self.ent) - 1, int(self.ent2 is not None))
        return head + self.items.tobytes() + self.item_ent.tobytes() + self.ent.tobytes() + (self.ent2.tobytes() if self.ent2 is not None else b"")

    # ---- the model ----

    def step_ids(self, ent=None):
        """The segment id of every step of the array the entries describe."""
        ent = self.ent if ent is None else ent
        pos = ent[:, 1].astype(np.int64)
        first = (ent[:-1, 0] & 0x7FFFFFFF).astype(np.int64)
        sign = np.where(ent[:-1, 0] >> 31, -1, 1).astype(np.int64)
        n = np.diff(pos)
        ids = np.zeros(int(pos[-1]), dtype=np.int64)
        at = np.repeat(pos[:-1], n)
        k = np.arange(pos[0], pos[-1]) - at
        ids[pos[0]:] = np.repeat(first, n) + np.repeat(sign, n) * k
        return ids

    def records(self, ent=None):
        """([(window, path, start, length - 1)], how many stretches leave [0, n_range)): every item's part of every entry it
        reads, cut at the window edges."""
        ent = self.ent if ent is None else ent
        ids, pos = self.step_ids(ent), ent[:, 1].astype(np.int64)
        out, dropped = [], 0
        for (b, e, _, path), (lo, hi) in zip(self.items.tolist(), self.item_ent.tolist()):
            for i in range(lo, hi):
                s, t = max(int(pos[i]), b), min(int(pos[i + 1]), e)
                if s >= t:
                    continue
                low, high = int(ids[s:t].min()), int(ids[s:t].max())
                assert high - low == t - s - 1
                if low < 0 or high >= self.n_range:
                    dropped += 1
                    continue
                for w in range(low >> self.wb, (high >> self.wb) + 1):
                    a, z = max(low, w << self.wb), min(high, ((w + 1) << self.wb) - 1)
                    out.append((w, path, a - (w << self.wb), z - a))
        return out, dropped

    def key_bits(self):
        bits = lambda n: max(1, (n - 1).bit_length())  # noqa: E731 (bits that hold 0 .. n - 1, one at the least)
        return self.wb + bits(self.n_paths) + bits(self.n_win)

    def model_verdict(self):
        """What the build says of the case, in the order it looks."""
        if not len(self.items) or not self.n_win:
            return "error"
        if self.key_bits() > 64:
            return "size"
        recs, dropped = self.records()
        if dropped:
            return "bounds"
        if not recs:
            return "size"
        if not self.waived and self.reserve >= 1 << 62:
            return "memory"
        if self.ent2 is not None:
            return "stale"
        return "built"

    def model_windows(self):
        """{window: its records (path, start, length - 1), ordered by path, start, length}."""
        by_win = collections.defaultdict(list)
        for w, path, s, l in self.records()[0]:
            by_win[w].append((path, s, l))
        return {w: sorted(v) for w, v in by_win.items()}

    def model_image(self):
        """win_chunk, rec, carry as the finaliser must leave them (for records of one start, in the model's order)."""
        wins = self.model_windows()
        win_chunk = np.zeros(self.n_win + 1, dtype=np.uint32)
        for w in range(self.n_win):
            win_chunk[w + 1] = win_chunk[w] + (len(wins.get(w, ())) + CHUNK - 1) // CHUNK
        rec = np.full(int(win_chunk[-1]) * CHUNK, PAD, dtype=np.uint32)
        carry = np.zeros(int(win_chunk[-1]), dtype=np.uint32)
        for w, rs in wins.items():
            at = int(win_chunk[w]) * CHUNK
            seen_end = {}
            for k, (path, s, l) in enumerate(rs):
                first = k == 0 or rs[k - 1][0] != path
                if k % CHUNK == 0:
                    flags = 0
                    carry[(at + k) // CHUNK] = 0 if first else seen_end[path]
                flags += first
                rec[at + k] = s | l << self.wb | (FIRST if first else 0) | flags << ORD_SHIFT
                seen_end[path] = max(seen_end.get(path, 0), s + l + 1)
        return win_chunk, rec, carry

    def kept_bytes(self):
        n_chunks = sum((len(v) + CHUNK - 1) // CHUNK for v in self.model_windows().values())
        return n_chunks * CHUNK * 4 + n_chunks * 4 + (self.n_win + 1) * 4

    def model_dump(self):
        """The bytes the program would write of an image that is the model's."""
        assert self.verdict == "built"
        win_chunk, rec, carry = self.model_image()
        n = sum(len(v) for v in self.model_windows().values())
        head = struct.pack("<8q", 1, 1, 3, self.kept_bytes(), 24 * n + 4 * (self.n_win + 1) + 16, len(carry), self.n_win, 0)
        return head + b"\0" * 16 + struct.pack("<q", 1) + win_chunk.tobytes() + rec.tobytes() + carry.tobytes()

    # ---- the checker ----

    def check(self, raw):
        d = Dump(raw)
        assert d.n_win == self.n_win, (d.n_win, self.n_win)
        assert d.polls and all(p == 0 for p in d.polls[:-1]) and d.polls[-1] == d.last, d.polls
        if self.verdict != "built":
            assert (d.last, d.phase, d.bytes, d.why) == (-1, -1, 0, self.verdict), (d.last, d.phase, d.bytes, d.why)
            assert d.n_chunks == 0 and d.win_chunk is None
            return
        assert (d.last, d.phase, d.why) == (1, 3, ""), (d.last, d.phase, d.why)
        wins = self.model_windows()
        n_records = sum(len(v) for v in wins.values())
        assert d.bytes == self.kept_bytes(), (d.bytes, self.kept_bytes())
        assert d.transient >= 24 * n_records + 4 * (self.n_win + 1) + 16, d.transient  # (the pairs in and out of the sort, the offsets; plus the sort's own scratch)
        want_chunk = np.zeros(self.n_win + 1, dtype=np.int64)
        for w, v in wins.items():
            want_chunk[w + 1] = (len(v) + CHUNK - 1) // CHUNK
        want_chunk = np.cumsum(want_chunk)
        assert (d.win_chunk == want_chunk).all(), ("win_chunk", np.flatnonzero(d.win_chunk != want_chunk)[:8])
        assert d.n_chunks == want_chunk[-1]
        wmask = (1 << self.wb) - 1
        for w, want in wins.items():
            c0, c1 = int(want_chunk[w]), int(want_chunk[w + 1])
            words = d.rec[c0 * CHUNK:c1 * CHUNK].astype(np.int64)
            n = len(want)
            assert (words[n:] == PAD).all(), (w, "padding", words[n:][words[n:] != PAD][:4])
            live = words[:n]
            assert not (live & PAD).any(), (w, "a record with the padding flag")
            assert not ((live & (FIRST - 1)) >> (self.wb + 10)).any(), (w, "bits between the length and the first-of-path flag")
            start, lenm1, first = live & wmask, (live >> self.wb) & 1023, (live & FIRST) != 0
            assert first[0], (w, "the window's first record begins a path")
            # the k-th stretch opened by a flag is the window's k-th path
            paths = sorted({p for p, _, _ in want})
            stretch = np.cumsum(first) - 1
            assert stretch[-1] + 1 == len(paths), (w, "paths", int(stretch[-1]) + 1, len(paths))
            got = sorted((paths[k], int(s), int(l)) for k, s, l in zip(stretch.tolist(), start.tolist(), lenm1.tolist()))
            assert got == want, (w, "records", [x for x in got if x not in want][:4], [x for x in want if x not in got][:4])
            same = ~first[1:]
            assert (start[1:][same] >= start[:-1][same]).all(), (w, "starts fall inside a path's stretch")
            # ordinals and carries, from the order found
            end = start + lenm1 + 1
            for c in range(c1 - c0):
                lo, hi = c * CHUNK, min((c + 1) * CHUNK, n)
                ord_want = np.cumsum(first[lo:hi])
                ord_got = (live[lo:hi] >> ORD_SHIFT) & ORD_MASK
                assert (ord_got == ord_want).all(), (w, c, "ordinal", ord_got.tolist(), ord_want.tolist())
                if first[lo]:
                    carry = 0
                else:
                    begin = int(np.flatnonzero(first[:lo])[-1])
                    carry = int(end[begin:lo].max())
                assert int(d.carry[c0 + c]) == carry, (w, c, "carry", int(d.carry[c0 + c]), carry)


class Dump:
    def __init__(self, raw):
        assert len(raw) >= 80, len(raw)
        n_polls, self.last, self.phase, self.bytes, self.transient, self.n_chunks, self.n_win, _ = struct.unpack_from("<8q", raw, 0)
        self.why = raw[64:80].split(b"\0")[0].decode()
        assert 1 <= n_polls <= 8
        self.polls = list(struct.unpack_from("<%dq" % n_polls, raw, 80))
        at = 80 + 8 * n_polls
        self.win_chunk = self.rec = self.carry = None
        if self.last == 1:
            want = at + 4 * (self.n_win + 1) + 4 * self.n_chunks * (CHUNK + 1)
            assert len(raw) == want, (len(raw), want)
            self.win_chunk = np.frombuffer(raw, dtype=np.uint32, count=self.n_win + 1, offset=at)
            at += 4 * (self.n_win + 1)
            self.rec = np.frombuffer(raw, dtype=np.uint32, count=self.n_chunks * CHUNK, offset=at)
            at += 4 * self.n_chunks * CHUNK
            self.carry = np.frombuffer(raw, dtype=np.uint32, count=self.n_chunks, offset=at)
        else:
            assert len(raw) == at, (len(raw), at)


# ---- the sweep and brute force (the CPU tests) ----

def sweep(case, win_chunk, rec, carry, order):
    """DESIGN.md section 3.3's sweep over an image, chunks in the order given: {cell: (depth, revisits)} for cells with depth."""
    w_of = np.repeat(np.arange(case.n_win), np.diff(win_chunk.astype(np.int64)))
    wsize, wmask = 1 << case.wb, (1 << case.wb) - 1
    D, Rv = {}, {}
    for c in order:
        w = int(w_of[c])
        if w not in D:
            D[w], Rv[w] = np.zeros(wsize + 1, dtype=np.int64), np.zeros(wsize + 1, dtype=np.int64)
        m = int(carry[c])  # the largest end among the path's earlier records
        for word in rec[c * CHUNK:(c + 1) * CHUNK].tolist():
            if word & PAD:
                continue
            if word & FIRST:
                m = 0
            s = word & wmask
            e = s + ((word >> case.wb) & 1023) + 1
            D[w][s] += 1
            D[w][e] -= 1
            if m > s:
                Rv[w][s] += 1
                Rv[w][min(e, m)] -= 1
            m = max(m, e)
    out = {}
    for w in D:
        d, r = np.cumsum(D[w])[:wsize], np.cumsum(Rv[w])[:wsize]
        for i in np.flatnonzero(d).tolist():
            out[(w << case.wb) + i] = (int(d[i]), int(r[i]))
    return out


def brute_force(case):
    """{cell: (depth, revisits)}: a cell a path covers c times has depth c and c - 1 revisits from that path."""
    ids = case.step_ids()
    per_path = collections.defaultdict(list)
    for b, e, _, path in case.items.tolist():
        per_path[path].append(ids[b:e])
    out = collections.defaultdict(lambda: [0, 0])
    for chunks in per_path.values():
        cells, cnt = np.unique(np.concatenate(chunks), return_counts=True)
        for i, c in zip(cells.tolist(), cnt.tolist()):
            out[i][0] += c
            out[i][1] += c - 1
    return {i: tuple(v) for i, v in out.items()}


# ---- the cases ----

def counts_of(case):
    return [len(case.model_windows().get(w, ())) for w in range(case.n_win)]


def flags_of(case):
    """(window, slot) of every first-of-path flag of the model's image."""
    win_chunk, rec, _ = case.model_image()
    at = np.flatnonzero((rec & FIRST) != 0)
    w_of = np.repeat(np.arange(case.n_win), np.diff(win_chunk.astype(np.int64)))
    return [(int(w_of[k // CHUNK]), int(k - int(win_chunk[w_of[k // CHUNK]]) * CHUNK)) for k in at.tolist()]


def window_runs(n, base, path):
    """Two paths' runs that put n records into the window at `base`: `path` 0 a run of 900 and short runs inside it (revisits),
    path 1 short runs over the same ids."""
    b = n // 3
    a = n - b
    if path == 1:
        return shorts(b, base)
    return ([R(base, 900)] if a else []) + shorts(max(a - 1, 0), base + 1)


def layout(b):
    w = 4096
    for path in (0, 1):
        runs = []
        for win, n in enumerate(LAYOUT_COUNTS):
            runs += window_runs(n, win * w, path)
        b.path(path, runs)


LAYOUT_COUNTS = [0, 1, 63, 0, 64, 65, 128, 129, 0]  # empty windows first, between and last


def lanes(b):
    for path in range(3):  # 64 records each: path 0 ends on lane 63, paths 1 and 2 begin on lane 0 of chunks 1 and 2
        b.path(path, [R(10 * path, 900)] + shorts(63, 1 + 10 * path))


def three_chunks(b):
    b.path(0, [R(0, 1000)] + shorts(149, 1))  # 150 records: chunk 1 is wholly path 0's, the largest end (1000) lies in chunk 0
    b.path(1, shorts(5, 400))


def under_way(b):
    b.path(0, [R(100, 800)] + shorts(69, 101))
    b.path(1, [R(50, 500)] + shorts(9, 60))
    b.path(2, shorts(5, 200) + [R(190, 40)])


def singles(n):
    def build(b):
        for p in range(n):
            b.path(p, [R(5 * p, 8)])
    return build


def equal_starts(b):
    b.path(0, shorts(62, 0) + [R(600, 5), R(600, 50), R(600, 20), R(600, 7), R(610, 3)])


def top_paths(b):
    for path in ((1 << 20) - 1, 0, (1 << 20) - 2):
        b.path(path, [R(100, 300), R(150, 20), R(4090, 12)])


def one_path(b):
    b.path(0, [R(100, 300), R(150, 20), R(100, 300), R(4090, 12), R(4000, 200)])


def descending(b):
    for path in range(5, -1, -1):
        b.path(path, [R(20 * path, 200), R(20 * path + 5, 10), R(4000 + path, 100)])


def three_items(b):
    b.path(0, [R(100, 300), R(500, 20)])
    b.path(1, [R(120, 50)])
    b.path(0, [R(150, 400), R(90, 20, True)])
    b.path(2, [R(4000, 200)])
    b.path(0, [R(100, 10), R(505, 3), R(4095, 2)])


def records_at(wb):
    w = 1 << wb

    def build(b):
        b.path(0, [R(w - 100, 200), R(2 * w + 49, 100, True),        # across a window edge, upward and downward
                   R(w - 700, 700), R(2 * w - 5, 5), R(2 * w - 1, 300, True),  # ending on a window's last cell (8192 at wb 13)
                   R(w, 50), R(2 * w, 10), R(w + 19, 20, True),      # starting on a window's first cell
                   R(10, 1024), R(w - 24, 1024), R(w + 1100, 1024, True), R(2 * w + 23, 1024, True)])  # exactly 1024 steps, inside a window and across an edge
        # a path cut into pieces inside its runs: a piece ends and the next begins inside an upward run (30 steps into the run
        # at 300), a downward one (at 700), and inside runs that cross an edge so that the clipped part crosses it as well
        runs = [R(100, 50), R(300, 80), R(w - 40, 80), R(2 * w - 40, 80), R(700, 80, True), R(w + 39, 80, True), R(2 * w + 39, 80, True), R(900, 5)]
        b.pieces(1, runs, [(1, 30), (2, 60), (3, 25), (4, 30), (5, 60), (6, 25)], slack=(1, 1))  # (slack: entries in a piece's range that its steps do not touch)
        b.path(2, [R(w - 50, 100), R(310, 40), R(680, 10)])
    return build


def many_items(n):
    def build(b):
        for p in range(n):
            b.path(p, [R(30 * p, 200), R(30 * p + 5, 10), R(30 * p + 3, 4)])
    return build


def many_entries(n):
    def build(b):
        b.path(0, [R(0, 1000)] + shorts(n - 1, 1))
        b.path(1, [R(3, 100)])
    return build


def far_windows(n_win):
    def build(b):
        w = 2048
        b.path(0, [R(10, 100), R(50, 20), R(8191 * w + 5, 300), R(8191 * w + 100, 20)] + ([R(8192 * w - 10, 30), R(8192 * w + 3, 40), R(8192 * w + 20, 5)] if n_win > 8192 else []))
        b.path(1, [R(8191 * w + 200, 50), R(0, 64)])
    return build


def plain(b):
    b.path(0, [R(100, 300), R(150, 20)])
    b.path(1, [R(4000, 200)])


def at_n_range(b):
    b.path(0, [R(100, 300), R(9000 - 5, 6)])  # the last id is n_range


def below_zero(b):
    b.path(0, [R(100, 300), R(5, 10, True)])


def touch_nothing(b):
    lo, hi, _, _ = b.lay([R(100, 50), R(300, 50)])
    b.lay([R(500, 50)])
    b.item(0, 110, 120, ent=(lo, lo + 1))  # (steps of the third run, entries of the first: every read inside the arrays)
    b.item(1, 100, 150, ent=(lo, hi))


def stale_first(b):
    b.path(0, [R(100, 300), R(4000, 50), R(150, 20)])


def stale_more(b):
    b.path(0, [R(100, 300), R(4070, 50), R(150, 20)])  # the second run now crosses a window edge: a record more than counted


def stale_fewer_first(b):
    b.path(0, [R(100, 300), R(4070, 50), R(150, 20)])


def stale_fewer(b):
    b.path(0, [R(100, 300), R(4000, 50), R(150, 20)])


def prop_layout(c):
    assert counts_of(c) == LAYOUT_COUNTS and c.n_range % 4096


def prop_lanes(c):
    assert counts_of(c)[0] == 192 and [s for w, s in flags_of(c) if w == 0] == [0, 64, 128]
    assert c.model_image()[2].tolist()[:3] == [0, 0, 0]


def prop_three_chunks(c):
    win_chunk, rec, carry = c.model_image()
    assert counts_of(c)[0] == 155 and [s for w, s in flags_of(c) if w == 0] == [0, 150]
    wmask = (1 << c.wb) - 1
    ends = (rec[64:128] & wmask) + ((rec[64:128] >> c.wb) & 1023) + 1
    assert ends.max() < 1000 and carry.tolist() == [0, 1000, 1000], "path 0's records fill chunk 1 entirely; its largest end lies in chunk 0"


def prop_under_way(c):
    assert [s for w, s in flags_of(c) if w == 0] == [0, 70, 80] and c.model_image()[2].tolist() == [0, 900]


def prop_singles(n):
    def prop(c):
        assert counts_of(c)[0] == n and len(flags_of(c)) == n
        rec = c.model_image()[1]
        assert int(rec[63] >> ORD_SHIFT) & ORD_MASK == 64 and (n == 64 or int(rec[64] >> ORD_SHIFT) & ORD_MASK == 1)
    return prop


def prop_equal_starts(c):
    rs = c.model_windows()[0]
    assert len(rs) == 67 and [s for _, s, _ in rs[62:66]] == [600] * 4 and len({l for _, _, l in rs[62:66]}) == 4


def prop_top_paths(c):
    assert c.key_bits() == 12 + 20 + 2 and sorted({p for p, _, _ in c.model_windows()[0]}) == [0, (1 << 20) - 2, (1 << 20) - 1]


def prop_one_path(c):
    assert c.key_bits() == 12 + 1 + 2 and len(flags_of(c)) == 2


def prop_descending(c):
    assert c.items[:, 3].tolist() == [5, 4, 3, 2, 1, 0]


def prop_three_items(c):
    assert c.items[:, 3].tolist() == [0, 1, 0, 2, 0] and [p for p, _, _ in c.model_windows()[0]] == [0] * 7 + [1] + [2]


def prop_records(wb):
    def prop(c):
        w = 1 << wb
        recs = c.records()[0]
        assert (0, 0, 10, 1023) in recs and (1, 0, 1100 - 1023, 1023) in recs, "runs of 1024 steps"
        assert (0, 0, w - 700, 699) in recs and (1, 0, w - 300, 299) in recs, "runs ending on the window's last cell"
        assert (1, 0, 0, 49) in recs and (2, 0, 0, 9) in recs and (1, 0, 0, 19) in recs, "runs starting on a window's first cell"
        assert (0, 0, w - 100, 99) in recs and (1, 0, 0, 99) in recs and (1, 0, w - 50, 49) in recs and (2, 0, 0, 49) in recs, "across an edge, both ways"
        assert (0, 0, w - 24, 23) in recs and (1, 0, 0, 999) in recs and (1, 0, w - 1000, 999) in recs and (2, 0, 0, 23) in recs
        # the pieces: upward at 300 cut 30 steps in; across edges with the clipped part crossing; downward likewise
        for r in [(0, 1, 300, 29), (0, 1, 330, 49), (0, 1, w - 40, 39), (1, 1, 0, 19), (1, 1, 20, 19), (1, 1, w - 40, 24), (1, 1, w - 15, 14), (2, 1, 0, 39),
                  (0, 1, 671, 29), (0, 1, 621, 49), (1, 1, 0, 39), (0, 1, w - 20, 19), (0, 1, w - 40, 19), (2, 1, 15, 24), (2, 1, 0, 14), (1, 1, w - 40, 39)]:
            assert r in recs, r
        assert len(c.items) == 9 and (c.item_ent[2:7, 1] - c.item_ent[2:7, 0] == 4).all(), "a piece reads an entry on either side that its steps do not touch"
    return prop


def prop_items(n):
    def prop(c):
        assert len(c.items) == n and c.n_cus == 1 and n > 8, "a workgroup of the grid of eight takes a second item"
    return prop


def prop_entries(n):
    def prop(c):
        assert int(c.item_ent[0, 1] - c.item_ent[0, 0]) == n and n > 256, "a lane takes a second entry"
    return prop


def prop_far(n_win):
    def prop(c):
        assert c.n_win == n_win and sorted(c.model_windows()) == ([0, 8191, 8192] if n_win > HIST_WINDOWS else [0, 8191])
    return prop


def built_cases():
    w = 4096
    out = [
        Case("layout", 12, 8 * w + 17, 2, layout, prop=prop_layout),
        Case("lanes_63_and_0", 12, 2 * w, 3, lanes, prop=prop_lanes),
        Case("three_chunks_one_path", 12, 2 * w, 2, three_chunks, prop=prop_three_chunks),
        Case("under_way_then_others", 12, w + 9, 3, under_way, prop=prop_under_way),
        Case("single_record_paths_64", 12, w, 64, singles(64), prop=prop_singles(64)),
        Case("single_record_paths_65", 12, w, 65, singles(65), prop=prop_singles(65)),
        Case("equal_starts_astride_a_seam", 12, w, 1, equal_starts, prop=prop_equal_starts),
        Case("n_paths_1", 12, 2 * w + 5, 1, one_path, prop=prop_one_path),
        Case("n_paths_2pow20", 12, 2 * w + 5, 1 << 20, top_paths, prop=prop_top_paths),
        Case("items_in_descending_path_order", 12, 2 * w, 6, descending, prop=prop_descending),
        Case("one_path_as_three_items", 12, 2 * w, 3, three_items, prop=prop_three_items),
    ]
    for wb in (11, 12, 13):
        out.append(Case("records_wb%d" % wb, wb, (2 << wb) + 57, 3, records_at(wb), prop=prop_records(wb)))
    out += [
        Case("items_9", 12, w, 9, many_items(9), prop=prop_items(9)),
        Case("items_17", 12, w, 17, many_items(17), prop=prop_items(17)),
        Case("entries_257", 12, w, 2, many_entries(257), prop=prop_entries(257)),
        Case("entries_513", 12, w, 2, many_entries(513), prop=prop_entries(513)),
        Case("windows_8192", 11, 8192 * 2048, 2, far_windows(8192), prop=prop_far(8192)),
        Case("windows_8193", 11, 8192 * 2048 + 100, 2, far_windows(8193), prop=prop_far(8193)),
        Case("memory_waived", 12, 9000, 2, plain, reserve=1 << 62, waived=True),
        Case("plain_two_cus", 12, 9000, 2, plain, n_cus=2),
    ]
    return out


def refused_cases():
    return [
        Case("bounds_id_at_n_range", 12, 9000, 1, at_n_range, verdict="bounds"),
        Case("bounds_below_segment_0", 12, 9000, 1, below_zero, verdict="bounds"),
        Case("size_no_records", 12, 9000, 2, touch_nothing, verdict="size", unchecked=True),
        Case("size_key_of_65_bits", 13, (1 << 32) - 1, (1 << 32) - 1, plain, n_win=1 << 20, verdict="size", unchecked=True),
        Case("memory", 12, 9000, 2, plain, reserve=1 << 62, verdict="memory"),
        Case("stale_more_than_counted", 12, 9000, 1, stale_first, second=stale_more, verdict="stale"),
        Case("stale_fewer_than_counted", 12, 9000, 1, stale_fewer_first, second=stale_fewer, verdict="stale"),
        Case("error_no_items", 12, 9000, 1, lambda b: b.lay([R(100, 50)]), verdict="error"),
    ]


def all_cases():
    """Every refusal stands between two cases that build: a refusal must leave the next build undisturbed."""
    built, refused = built_cases(), refused_cases()
    assert len(built) > len(refused)
    out = []
    for k, c in enumerate(built):
        out.append(c)
        if k < len(refused):
            out.append(refused[k])
    return out


CASES = all_cases()
