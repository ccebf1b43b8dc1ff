"""The pangenotype model (tests/gaf_model.py) against the reference's known answer and hand-derived rows, and the
argument checks of the C ABI, which need no device."""
import ctypes
import os

import numpy as np
import pytest

import gaf_model as gm
import gaf_shapes as gs
import pollen_amd as pa
from conftest import GOLDEN
from pollen_amd import _lib

GAF = os.path.join(GOLDEN, "gaf")
TINY = [1, 2, 3, 4]  # ref_tiny.gfa's segment names, in id order (sequential: id = name - 1)
T, F = True, False


def read(name):
    with open(os.path.join(GAF, name), "rb") as f:
        return f.read()


def test_known_answer_of_the_reference():
    # flatgfa-py/test/test_matrix.py:11-18
    assert gm.matrix([read("tiny.gaf"), read("tiny2.gaf")], TINY) == [[T, T, T, T], [T, T, F, T]]
    assert gm.table([read("tiny2.gaf")], TINY) == b"1101\n"


def fields(path_field: bytes, rest: bytes = b"\t150\t0\t150\t150\t150\t60\tcg:Z:150M") -> bytes:
    return b"read\t150\t0\t150\t+\t" + path_field + rest + b"\n"


EDGE_LINES = {
    "hash_line": (b"#read\t150\t0\t150\t+\t>1\t150\n", [F, F, F, F]),
    "empty_line": (b"\n" + fields(b">2"), [F, T, F, F]),
    "crlf": (b"read\t150\t0\t150\t+\t>3\r\n", [F, F, T, F]),
    "fewer_than_five_tabs": (b"read\t150\t0\t150\t>1>2\n", [F, F, F, F]),
    "fifth_tab_last": (b"read\t150\t0\t150\t+\t\n", [F, F, F, F]),
    "empty_path_field": (b"read\t150\t0\t150\t+\t\t>1\t>2\n", [F, F, F, F]),
    "stable_ids": (fields(b"chr1:100-250"), [F, F, F, F]),
    "junk_between_tokens": (fields(b">1x<2"), [T, T, F, F]),
    "leading_zeros": (fields(b">0004<003"), [F, F, T, T]),
    "last_line_without_newline": (fields(b">2") + b"read\t150\t0\t150\t+\t>99", [F, T, F, F]),
    "wraps_mod_2_64": (fields(b">18446744073709551617"), [T, F, F, F]),
    "orientation_ignored": (fields(b"<4<4>4"), [F, F, F, T]),
    "seventh_column_not_read": (b"read\t150\t0\t150\t+\t>1\t>2>3\n", [T, F, F, F]),
}


@pytest.mark.parametrize("name", sorted(EDGE_LINES))
def test_edge_lines(name):
    text, want = EDGE_LINES[name]
    assert gm.row(text, TINY) == want


def test_edges_fixture():
    # tests/golden/gaf/edges.gaf: the edge lines in one file, ending in a line without '\n' that names no segment
    assert gm.row(read("edges.gaf"), TINY) == [T, T, T, T]
    assert gm.row(read("edges.gaf").replace(b">0004", b">0002"), TINY) == [T, T, T, F]


@pytest.mark.parametrize("path_field", [b">", b"<1>"], ids=["no_digits", "trailing_bare"])
def test_name_zero_is_an_error(path_field):
    text = fields(b">1") + fields(path_field)
    with pytest.raises(gm.GafError) as e:
        gm.row(text, TINY, file=3)
    assert (e.value.file, e.value.offset) == (3, len(fields(b">1")))


def test_unknown_name_is_an_error():
    text = fields(b">1") + b"#comment\n" + fields(b">2>5")
    with pytest.raises(gm.GafError) as e:
        gm.row(text, TINY)
    assert e.value.offset == len(fields(b">1")) + len(b"#comment\n")


def test_unknown_name_in_a_skipped_place_is_not_an_error():
    text = b"#read\t1\t1\t1\t+\t>9\n" + b"read\t1\t1\t1\t>9\n" + fields(b">1", b"\t>9") + b"read\t1\t1\t1\t+\t>9"
    assert gm.row(text, TINY) == [T, F, F, F]


def test_non_sequential_names():
    # edge_names_loops.gfa: names 10, 5, 7, 1, 2 -- none sequential from the first, so all of them are `others`
    names = [10, 5, 7, 1, 2]
    assert gm.name_map(names) == (0, {10: 0, 5: 1, 7: 2, 1: 3, 2: 4})
    assert gm.row(fields(b">1<10>2"), names) == [T, F, F, T, T]
    # a sequential run, then a break, then a duplicate that replaces the earlier id (namemap.rs:23)
    assert gm.name_map([1, 2, 3, 9, 4, 9]) == (3, {9: 5, 4: 4})
    assert gm.row(fields(b">9>4>3"), [1, 2, 3, 9, 4, 9]) == [F, F, T, F, T, T]


def test_matrix_rows_are_per_file():
    assert gm.matrix([b"", read("tiny2.gaf"), read("tiny2.gaf")], TINY) == [[F] * 4, [T, T, F, T], [T, T, F, T]]


def test_abi_rejects_null_arguments_without_a_device():
    lib = _lib.lib()
    one = (ctypes.c_size_t * 1)(4)
    bits = (ctypes.c_uint64 * 1)()
    assert lib.flatgfa_pangenotype_matrix(None, None, None, 0, None) == -1
    g = pa.parse(os.path.join(GOLDEN, "ref_tiny.gfa"))
    try:
        assert lib.flatgfa_pangenotype_matrix(g._h, None, one, 1, bits) == -1
        assert lib.flatgfa_pangenotype_matrix(g._h, (ctypes.c_void_p * 1)(None), one, 1, bits) == -1  # a length with no text
        assert lib.flatgfa_pangenotype_matrix(g._h, (ctypes.c_void_p * 1)(None), one, 1, None) == -1
        assert "pangenotype_matrix" in _lib.last_error()
        assert lib.flatgfa_pangenotype_table(g._h, None, None, 0, None, None) == -1
        assert lib.flatgfa_dev_pangenotype_row(None, None, 16, None, None, None) == -1
        assert lib.flatgfa_dev_pangenotype_row(g._h, None, 16, None, None, None) == -1
    finally:
        g.close()


# ---- row_fast (a line at a time) pinned to row (a byte at a time) ----

def test_digits_mod_2_64():
    for s in (b"", b"0", b"000", b"7", b"0018446744073709551615", b"18446744073709551616", b"9" * 19, b"9" * 20,
              b"1234567890123456789012345"):
        assert gm.digits_mod_2_64(s) == int(s or b"0") % (1 << 64), s
    # past int()'s default limit on digit strings (4 300)
    assert gm.digits_mod_2_64(b"0" * 100_000 + b"47") == 47
    assert gm.digits_mod_2_64(b"1" + b"0" * 5000) == pow(10, 5000, 1 << 64)
    assert gm.digits_mod_2_64(b"3" * 4999) == sum(3 * pow(10, i, 1 << 64) for i in range(4999)) % (1 << 64)


def outcome(fn, texts, names):
    try:
        return fn(texts, names)
    except gm.GafError as e:
        return ("error", e.file, e.offset)


def soup(rng, names, n, unknown):
    """Bytes from the alphabet the rules look at, in runs, naming known segments (and, one token in `unknown`, a name
    the graph lacks)."""
    pieces = [b"\t", b"\n", b"\n\n", b"#", b"x", b"\r\n", b"\t\t\t\t\t"]
    out, size = [], 0
    while size < n:
        k = int(rng.integers(0, len(pieces) + 4))
        if k < len(pieces):
            out.append(pieces[k])
        elif unknown and rng.integers(unknown) == 0:
            out.append(b"<%d" % int(rng.integers(0, 60)) if k % 2 else b">")
        else:
            out.append((b">0%d" if k % 3 else b"<%d") % names[int(rng.integers(len(names)))])
        size += len(out[-1])
    return b"".join(out)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("seed", range(6))
def test_row_fast_matches_row_on_tile_shapes(tile, seed):
    # every generator of tests/gaf_shapes.py with tiny tiles, each alone, all in one text in shuffled order, and in several
    # texts of one matrix; the shapes' own claims (names they set, the error offset) hold for both models
    shapes = gs.good_shapes(tile, seed) + gs.bad_shapes(tile, seed)
    idx = {n: i for i, n in enumerate(gs.NAMES)}
    for label, sh in shapes:
        want = outcome(gm.matrix, [sh.text], gs.NAMES)
        assert outcome(gm.matrix_fast, [sh.text], gs.NAMES) == want, label
        if sh.bad is not None:
            assert want == ("error", 0, sh.bad), label
            continue
        assert not isinstance(want, tuple), (label, want)
        got = {n for n in gs.NAMES if want[0][idx[n]]}
        assert sh.sets <= got and (not sh.exact or got == sh.sets), label
    rng = np.random.default_rng(seed)
    good = [sh.text for _, sh in shapes[:-2]]
    mixed = b"".join(good[int(i)] for i in rng.permutation(len(good)))
    texts = [mixed, b"", good[0]]
    assert outcome(gm.matrix_fast, texts, gs.NAMES) == outcome(gm.matrix, texts, gs.NAMES)
    g_text = shapes[-2][1].text
    texts = [mixed, g_text + mixed, g_text]
    want = outcome(gm.matrix, texts, gs.NAMES)
    assert want == ("error", 1, shapes[-2][1].bad)
    assert outcome(gm.matrix_fast, texts, gs.NAMES) == want


@pytest.mark.parametrize("seed", range(100))
def test_row_fast_matches_row_on_byte_soup(seed):
    rng = np.random.default_rng(1000 + seed)
    names = [int(x) for x in rng.permutation([1, 2, 3, 4, 5, 6, 977, 2**63, 2**64 - 1, 0, 5, 40])[:int(rng.integers(4, 12))]]
    text = soup(rng, [n for n in names if n] + [18446744073709551617] * (1 in names), int(rng.integers(50, 3000)), seed % 3 * 40)
    assert outcome(gm.matrix_fast, [text], names) == outcome(gm.matrix, [text], names)


@pytest.mark.parametrize("name", sorted(EDGE_LINES))
def test_row_fast_on_edge_lines(name):
    text, want = EDGE_LINES[name]
    assert gm.row_fast(text, TINY) == want
