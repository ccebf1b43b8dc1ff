"""The pangenotype model (tests/gaf_model.py) against the reference's known answer and hand-derived rows, and the
argument checks of the C ABI, which need no device."""
import ctypes
import os

import pytest

import gaf_model as gm
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
