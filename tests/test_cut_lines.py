"""fgfa::cut_lines -- the one chunker behind the pangenotype matrix and the GAF lookup (DESIGN.md sections 9 and 11) --
against a chunker of a few lines written here.  `host_check --cut-lines TARGET FILE` (tests/host_check/host_check.cpp)
prints the pieces; the plain build is enough here, tests/test_host_sanitized.py runs the same function under the sanitizers.
No GPU needed."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
EXE = os.path.join(ROOT, "pollen_amd", "build", "host_check")


@pytest.fixture(scope="module")
def host_check():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    subprocess.run(["make", "-C", CSRC, "host_check"], check=True, capture_output=True, timeout=600)
    return EXE


def model(text: bytes, target: int):
    """Pieces [begin, end): each ends behind a newline and holds as many whole lines as fit `target` bytes -- one line,
    however long, where none fits.  Nothing behind the last newline is in a piece."""
    end = text.rfind(b"\n") + 1
    pieces, b = [], 0
    while b < end:
        e = text.index(b"\n", b) + 1  # the first line, always
        while e < end and text.index(b"\n", e) + 1 - b <= target:
            e = text.index(b"\n", e) + 1
        pieces.append((b, e))
        b = e
    return pieces


def cut(exe, tmp_path, text: bytes, target: int):
    path = tmp_path / "text"
    path.write_bytes(text)
    r = subprocess.run([exe, "--cut-lines", str(target), str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]


T = 8  # the target the texts below are written around
CASES = {
    "empty": (b"", T),
    "no newline at all": (b"abcdefghijkl", T),
    "a single newline": (b"\n", T),
    "a tail without a newline is dropped": (b"abc\ndef\nghi", T),
    "a line of exactly target bytes with its newline": (b"abcdefg\nhi\n", T),
    "a line of target + 1 bytes grows its piece": (b"abcdefgh\nhi\n", T),
    "a line of target + 1 bytes behind a short one": (b"ab\nabcdefgh\nhi\n", T),
    "a long line that is the last line": (b"ab\ncd\nabcdefghijklmnopqrstuvwxyz\n", T),
    "a long last line with a tail behind it": (b"ab\nabcdefghijklmnopqrstuvwxyz\ntail", T),
    "a newline at byte target - 1 of a piece": (b"abc\ndef\nghi\n", T),
    "a newline at byte target of a piece": (b"abc\ndefg\nhi\n", T),
    "a newline at byte target - 1 and at byte target": (b"abcdefg\n\nhi\n", T),
    "target 1": (b"a\n\nbc\n\n\nd", 1),
    "target 1, empty lines only": (b"\n\n\n", 1),
    "target equal to the whole length": (b"abc\ndef\nghi\n", 12),
    "target equal to the whole length, with a tail": (b"abc\ndef\ngh", 10),
    "target larger than the text": (b"abc\ndef\nghi\n", 1000),
    "many short lines": (b"a\n" * 40, T),
}


def test_the_model_on_cases_worked_by_hand():
    assert model(b"abc\ndef\nghi\n", T) == [(0, 8), (8, 12)]       # the newline at byte 7 closes a full piece
    assert model(b"abc\ndefg\nhi\n", T) == [(0, 4), (4, 12)]       # the one at byte 8 does not fit
    assert model(b"abcdefgh\nhi\n", T) == [(0, 9), (9, 12)]        # a line of 9 bytes is a piece of 9
    assert model(b"ab\nabcdefgh\nhi\n", T) == [(0, 3), (3, 12), (12, 15)]
    assert model(b"abc\ndef\nghi", T) == [(0, 8)]
    assert model(b"abc", T) == [] and model(b"", T) == [] and model(b"\n", T) == [(0, 1)]
    assert model(b"a\n\nbc\n", 1) == [(0, 2), (2, 3), (3, 6)]


@pytest.mark.parametrize("name", list(CASES))
def test_pieces_match_the_model_and_tile_the_lines(host_check, tmp_path, name):
    text, target = CASES[name]
    got = cut(host_check, tmp_path, text, target)
    assert got == model(text, target)
    # the pieces tile [0, last newline + 1): no gap, no overlap, nothing of the tail
    at = 0
    for b, e in got:
        assert b == at and e > b and text[e - 1:e] == b"\n"
        assert e - b <= target or text.count(b"\n", b, e) == 1
        at = e
    assert at == text.rfind(b"\n") + 1
