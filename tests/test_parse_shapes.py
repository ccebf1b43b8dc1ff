"""The plain grammar of the device GFA parser, restated in tests/parse_shapes.py, against the texts the suite has: every
golden GFA and every handmade text is plain (so the GPU tests may demand the device route for them), and of the parser
quirks exactly the listed ones are not.  The shapes' own assertions run for a tile of 4096 bytes.  No GPU needed."""
import numpy as np
import pytest

import pollen_amd as pa
import parse_shapes as ps
from test_host import QUIRKS


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("gfa", ps.all_golden_gfas(), ids=ps.golden_id)
def test_goldens_are_plain(gfa):
    text = read(gfa)
    assert ps.reason(text) == "plain" and ps.reason(text, True) == "plain"


def test_there_are_69_goldens_and_one_lacks_its_last_newline():
    texts = [read(g) for g in ps.all_golden_gfas()]
    assert len(texts) == 69
    assert [ps.golden_id(g) for g, t in zip(ps.all_golden_gfas(), texts) if not t.endswith(b"\n")] == ["ref_handmade_no-test-flip4"]


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade_texts_are_plain(name):
    assert ps.plain(ps.HANDMADE[name]) and ps.plain(ps.HANDMADE[name], True)


def test_quirks_the_grammar_excludes():
    assert len(QUIRKS) == 30
    got = {i: ps.reason(t) for i, t in enumerate(QUIRKS) if not ps.plain(t)}
    assert got == ps.QUIRKS_NOT_PLAIN
    assert {i: ps.reason(t) for i, t in enumerate(ps.ADDED) if not ps.plain(t)} == ps.ADDED_NOT_PLAIN


def test_plain_quirks_parse_on_the_host():
    """A plain text is one the host parser accepts: the device route never hides an error."""
    for t in QUIRKS + ps.ADDED:
        for stream in (False, True):
            if ps.plain(t, stream):
                (pa.parse_stream_bytes if stream else pa.parse_bytes)(t)


def test_stream_mode_sees_the_last_line():
    assert ps.plain(b"S\t1\tA\nX") and ps.reason(b"S\t1\tA\nX", True) == "grammar"
    assert ps.plain(b"S\t1\tA\nP\tp\t2+\t*") and ps.reason(b"S\t1\tA\nP\tp\t2+\t*", True) == "name"
    assert ps.lines_of(b"", True) == [] and ps.lines_of(b"S\t1\tA\n", True) == [b"S\t1\tA"]


def test_limits_and_precedence():
    long_name = b"0" * 32 + b"7"
    assert ps.reason(b"S\t" + long_name + b"\tA\n") == "limit"
    assert ps.plain(b"S\t" + long_name[1:] + b"\tA\n")                           # 32 digits are read
    assert ps.reason(b"S\t1\tA\nP\tp\t" + long_name + b"+\t*\n") == "limit"      # (before its name is looked up)
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t" + long_name + b"M\n") == "limit"
    assert ps.reason(b"S\t" + long_name + b"\tA\nX\n") == "grammar"              # grammar first
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t4294967297M\n") == "plain"        # parse_num::<u32> wraps to 1
    assert ps.reason(b"S\t1\tA\nL\t1\t+\t1\t+\t256M\n") == "grammar"
    assert ps.reason(b"S\t0\tA\nP\tp\t0+\t*\n") == "name"                        # name 0 never resolves (namemap.rs:28)


def test_shapes_hold_for_a_4_kib_tile():
    T = 4096
    for k in range(-1, 8):
        assert ps.plain(ps.item_on_edge(T, k))
    for make in (ps.field_begins_on_tile, ps.field_ends_on_tile, ps.short_lines_in_one_tile, ps.line_across_tiles,
                 ps.newline_ends_tile, ps.newline_begins_tile):
        text = make(T)
        assert ps.plain(text) and ps.plain(text, True)
        pa.parse_bytes(text)
    for text in (ps.many_short_paths(), ps.reversed_names(), ps.skipped_names(), ps.duplicate_names(T, True),
                 ps.duplicate_names(T, False), ps.digit_names()):
        assert ps.plain(text)
        pa.parse_bytes(text)
    assert [len(ps.steps_exact(n)) for n in (5, 6, 7, 100)] == [5, 6, 7, 100]


def test_normalized_pools():
    """The identity, but for the line order, on a text in normalized order; an empty alignment becomes the printer's 0M."""
    for text in (ps.HANDMADE["only a header"], b"H\tVN:Z:1.0\nS\t1\tA\nS\t2\tC\nP\tp\t1+,2-\t2M,1M3D\nP\tq\t2+\t*\nL\t1\t+\t2\t-\t4M\nL\t2\t+\t1\t+\t0M\n"):
        with pa.parse_bytes(text) as g:
            want = ps.pools_of(g)
            want["line_order"] = b""
            assert ps.normalized_pools(g) == want
    # file order L, P: the link's ops move behind the path's; a link without ops gets one
    with pa.parse_bytes(b"S\t1\tA\nL\t1\t+\t1\t-\t\nL\t1\t-\t1\t+\t7M\nP\tp\t1+,1-\t2M\n") as g:
        assert (g.pool("alignment") >> 8).tolist() == [7, 2]
        n = ps.normalized_pools(g)
        assert np.frombuffer(n["alignment"], "<u4").tolist() == [2 << 8, 0, 7 << 8]
        assert np.frombuffer(n["links"], "<u4").reshape(-1, 4)[:, 2:].tolist() == [[1, 2], [2, 3]]
        assert np.frombuffer(n["overlaps"], "<u4").tolist() == [0, 1]


# ---- the seam shapes of tests/test_gpu_parse_seams.py: their geometry at T = 4096 and their classes ----

T = 4096
HOST = {False: pa.parse_bytes, True: pa.parse_stream_bytes}
OUTCOME = {("plain", "accepts"): "plain", ("limit", "accepts"): "accepted", ("grammar", "accepts"): "accepted",
           ("grammar", "error"): "error", ("name", "error"): "error"}


def outcomes(text):
    return [ps.outcome(text, stream, HOST[stream]) for stream in (False, True)]


@pytest.mark.parametrize("item", list(ps.STEP_ITEMS), ids=repr)
def test_step_items_keep_their_class_wherever_they_lie(item):
    why, host = ps.STEP_ITEMS[item]
    for x in (T, T + ps.LANE):
        for k in range(-1, len(item) + 1):
            text = ps.on_edge(T, x, k, item)
            assert (ps.reason(text), ps.reason(text, True)) == (why, why), (x, k)
            assert outcomes(text) == [OUTCOME[why, host]] * 2, (x, k)


@pytest.mark.parametrize("item", list(ps.FIELD_ENDS), ids=repr)
def test_field_ends_keep_their_class_wherever_they_lie(item):
    why, host = ps.FIELD_ENDS[item]
    for x in (T, T + ps.LANE):
        for k in range(-1, len(item) + 1):
            text = ps.on_edge(T, x, k, item, ps.FIELD_END_TAIL)
            assert (ps.reason(text), ps.reason(text, True)) == (why, why), (x, k)
            assert outcomes(text) == [OUTCOME[why, host]] * 2, (x, k)


def test_on_edge_generalises_item_on_edge():
    assert ps.on_edge(T, T, 3, b"12345+,").index(b"12345+,") == T - 3
    assert ps.on_edge(T, T + 16, -1, b"1+,,")[T + 16:T + 22] == b",1+,,1"
    assert sum(why == "grammar" and host == "accepts" for why, host in ps.FIELD_ENDS.values()) == 6


def test_cigar_exact():
    assert ps.cigar_exact(0) == b"" and ps.cigar_exact(1) is None and ps.cigar_exact(0, True) is None and ps.cigar_exact(1, True) == b"*"
    for commas in (False, True):
        for n in range(2, 300):
            field = ps.cigar_exact(n, commas)  # (asserts its length and its form)
            assert all(int(d) <= 255 for d in ps._OP.findall(field))
            assert (b"," in field) == (commas and n >= 8)
        field = ps.cigar_exact(ps.CIGAR_LEN, commas)
        assert {len(d) for d in ps._OP.findall(field)} == {1, 2, 3} and all(c in field for c in b"MNDI")
        text = ps.cigar_text(field, commas)
        assert ps.plain(text) and ps.plain(text, True)


def test_cigar_faults_come_in_every_class():
    family = ps.cigar_family()
    assert len(family) == 2 * (len(ps.FAULT_AT) * len(ps.FAULT_EDITS) + len(ps.CIGAR_STRADDLES))
    got = {name: outcomes(text) for name, text in family.items()}
    assert all(a == b for a, b in got.values())  # (every text ends in a newline: one class in both modes)
    for form in "LP":
        count = {c: sum(v[0] == c for name, v in got.items() if name[0] == form) for c in ("plain", "accepted", "error")}
        print(form, count)
        assert min(count.values()) >= 5, count
    why = {name: ps.reason(text) for name, text in family.items()}
    for form, comma in (("L", "grammar"), ("P", "plain")):
        assert why[form + ": 256M, the 2 at byte 63"] == why[form + ": 256M, the M at byte 64"] == "grammar"
        assert why[form + ": 255M, the 2 at byte 63"] == "plain"
        assert [why["%s: %d digits, %s" % (form, d, w)] for d in (33, 32) for w in ("16 before byte 64", "the M at byte 64")] == ["limit"] * 2 + ["plain"] * 2
        assert [why["%s: %s byte 128" % (form, w)] for w in ("33 digits, 16 before", "33 digits, the M at", "32 digits, the M at")] == ["limit", "limit", "plain"]
        assert why[form + ": 33 digits, one before byte 64"] == why[form + ": 33 digits worth 256, 16 before byte 64"] == "limit"
        assert why[form + ": 32 digits worth 256, 16 before byte 64"] == "grammar"
        assert why[form + ": an op letter at byte 64 behind one"] == why[form + ": a comma at byte 63, a letter at 64"] == "grammar"
        assert why[form + ": a comma at byte 64"] == why[form + ": a comma at byte 128"] == comma
    # what lies at the wave's seams in the field every edit is made in
    for commas in (False, True):
        line = ps.cigar_fault(64, b"x", commas).split(b"\n")[2]
        assert line.split(b"\t")[-1][64:65] == b"x" and len(line.split(b"\t")[-1]) == 200


def test_field_ladder_is_plain_and_the_host_parser_takes_it():
    text = ps.field_ladder()  # (asserts its lengths)
    assert 50_000 < len(text) < 80_000
    assert ps.plain(text) and ps.plain(text, True)
    for stream in (False, True):
        with HOST[stream](text) as g:
            segs, paths = g.pool("segs"), g.pool("paths")
            assert set((segs["seq_end"] - segs["seq_start"]).tolist()) == set(ps.LADDER)
            assert set((segs["opt_end"] - segs["opt_start"]).tolist()) == set(ps.LADDER)
            assert set((paths["name_end"] - paths["name_start"]).tolist()) >= set(ps.LADDER)
    assert all(n in ps.STRETCHES for n in (2, 5, 60, 63, 64, 65, 70, 124, 127, 128, 129, 132))


def test_line_index_texts():
    texts = ps.line_index_texts(T)  # (each asserts where its fault lies)
    assert {name: ps.reason(t) for name, t in texts.items()} == {
        "kind X at byte T - 1": "grammar", "kind X at byte T": "grammar", "no tab at byte T": "grammar", "an empty line across T": "grammar",
        "a second header at T": "grammar", "the one header at T": "plain"}
    for t in texts.values():
        assert ps.reason(t, True) == ps.reason(t)
    for r in range(16):
        for fault in (False, True):
            text = ps.unterminated(T, r, fault)
            assert len(text) % 16 == r and ps.plain(text) and ps.reason(text, True) == ("grammar" if fault else "plain")
            with pa.parse_bytes(text) as g:
                assert g.path_count == 0
        with pa.parse_stream_bytes(ps.unterminated(T, r, False)) as g:
            assert g.path_count == 1
    for kind in b"SPLH":
        text = ps.lone_kind(T, bytes([kind]))
        assert ps.plain(text) and ps.reason(text, True) == "grammar"


def test_precedence_texts():
    pairs, triples = ps.precedence_pairs(), ps.precedence_triples()
    assert len(pairs) == 5 * 4 + 5 * 2 + 4 * 2 and len(triples) == 5 * 4 * 2
    for cls, faults in ps.FAULTS.items():  # every fault alone is of its class, in whichever tile
        for k, line in enumerate(faults.values()):
            text = ps.faults_in_tiles(T, {k % 3: line})
            assert ps.reason(text) == ps.reason(text, True) == cls, line
    assert all(max(map(len, ps.re.findall(rb"[0-9]+", line))) == ps.WINDOW + 1 for line in ps.FAULTS["limit"].values())
    assert ps.plain(ps.faults_in_tiles(T, {}))
    HOST[False](ps.faults_in_tiles(T, {})).close()
    for k, (ca, la, cb, lb) in enumerate(pairs.values()):
        first = min(ca, cb, key=ps.PRECEDENCE.index)
        ab, ba = ps.pair_texts(T, k, la, lb)
        assert ab != ba and ab.index(la) < ab.index(lb) and ba.index(lb) < ba.index(la)
        assert ab.index(la) // T != ab.index(lb) // T
        assert ps.reason(ab) == ps.reason(ba) == ps.reason(ab, True) == first
    for lines in triples.values():
        texts = ps.triple_texts(T, *lines)
        assert len(set(texts)) == 6 and all(ps.reason(t) == "grammar" for t in texts)
        assert all(sorted(t.index(ln) // T for ln in lines) == [0, 1, 2] for t in texts)


def test_small_texts():
    """Every text of at most 5 bytes over S, tab, 1 and newline, and every proper prefix of the handmade texts: what is plain,
    the host parser accepts."""
    texts = ps.small_texts()
    assert len(texts) == 1365
    for text in texts + ps.handmade_prefixes():
        for stream in (False, True):
            if ps.plain(text, stream):
                HOST[stream](text).close()
    assert sum(ps.plain(t, s) for t in texts for s in (False, True)) == 372
    assert len(ps.handmade_prefixes()) == sum(map(len, ps.HANDMADE.values()))


@pytest.mark.parametrize("what", list(ps.LIMIT_TEXTS))
def test_limit_texts_have_one_largest_quantity(what):
    text = ps.LIMIT_TEXTS[what]
    assert ps.plain(text) and ps.plain(text, True)
    with pa.parse_bytes(text) as g:
        q = ps.quantities(ps.pools_of(g))
    assert set(q) == {"lines", "header", "segs", "paths", "links", "steps", "seq_data", "overlaps", "alignment", "name_data", "optional_data"}
    top = max(q.values())
    assert q[what] == top >= 7
    assert [name for name, v in q.items() if v == top] == ([what] if what != "overlaps" else ["overlaps", "alignment"])
