"""`fgfa bed -a A -b B` as the reference computes it, rule by rule: the parser of flatgfa/src/flatbed.rs:125-158 over the line
splitter of memfile.rs:51-63, and the double loop of cli/cmds.rs:404-412 over FlatBED::get_intersects (flatbed.rs:37-57).  No
pruning, no grouping: every entry of A against every entry of B.  The yardstick of the GPU tests."""
U64 = (1 << 64) - 1


class BedError(Exception):
    pass


def _number(line: bytes, at: int):
    """Digits from `at` on as a wrapping u64; (value, where they end).  No digit: the reference panics."""
    v, k = 0, at
    while k < len(line) and 48 <= line[k] <= 57:
        v = (v * 10 + line[k] - 48) & U64
        k += 1
    if k == at:
        raise BedError("BED: expected number")
    return v, k


def parse(text: bytes):
    """[(name, start, end)] of BED text."""
    out = []
    lines = bytes(text).split(b"\n")[:-1]  # an unterminated last line is dropped
    for line in lines:
        if line[:1] == b"#":
            continue
        tab = line.find(b"\t")
        name = line if tab < 0 else line[:tab]  # the bytes before the first tab; may be empty
        start, k = _number(line, len(line) if tab < 0 else tab + 1)
        if k >= len(line):
            raise BedError("BED: line ends after the start column")
        end, _ = _number(line, k + 1)  # columns after the third are ignored
        out.append((name, start, end))
    return out


def pairs(a_entries, b_entries):
    """[(a index, b index, s, e)] in the reference's order: every a in file order, for each every x of b in file order."""
    out = []
    for i, (an, a0, a1) in enumerate(a_entries):
        for k, (xn, x0, x1) in enumerate(b_entries):
            s = a0 if x0 < a0 else x0
            e = a1 if a1 < x1 else x1
            if an == xn and e > s:
                out.append((i, k, s, e))
    return out


def intersect(a: bytes, b: bytes) -> bytes:
    ea, eb = parse(a), parse(b)
    return b"".join(b"%s\t%d\t%d\n" % (eb[k][0], s, e) for _, k, s, e in pairs(ea, eb))


def grouped(entries):
    """B as the device takes it: (ids, order) -- dense ids in order of first appearance, and the entries' indices grouped by
    id, file order kept inside a group."""
    ids = {}
    for name, _, _ in entries:
        ids.setdefault(name, len(ids))
    order = sorted(range(len(entries)), key=lambda k: ids[entries[k][0]])  # (sorted is stable)
    return ids, order
