"""tests/sorted_image_cases.py without a GPU: every case states what it is for and the model's image of it is right.

For every case that builds, the model's image -- chunks, first-of-path flags, padding, carry words -- is swept as DESIGN.md
section 3.3 says (a running maximum of a path's earlier ends, seeded by the chunk's carry), chunk by chunk in a shuffled order,
and depth and revisits per cell must be brute force's over the case's paths: a cell a path covers c times counts c - 1 revisits.
So a model that lays records, flags or carries out wrongly fails here, before it is held against the device.  Every case also
asserts its stated property (`prop`), and the checker must pass the model's own image and notice each single wrong word in it.
"""
import numpy as np
import pytest

import sorted_image_cases as sc

BUILT = [c for c in sc.CASES if c.verdict == "built"]


def test_every_case_has_its_own_id():
    assert len({c.id for c in sc.CASES}) == len(sc.CASES)


def test_every_refusal_stands_between_two_builds():
    assert sc.CASES[0].verdict == "built" and sc.CASES[-1].verdict == "built"
    for a, b in zip(sc.CASES, sc.CASES[1:]):
        assert a.verdict == "built" or b.verdict == "built", (a.id, b.id)
    assert {c.verdict for c in sc.CASES} == {"built", "bounds", "size", "memory", "stale", "error"}


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_the_models_verdict_is_the_cases(case):
    assert case.model_verdict() == case.verdict
    if case.ent2 is not None:
        first, second = len(case.records()[0]), len(case.records(case.ent2)[0])
        assert (second > first) == ("more" in case.id) and second != first


@pytest.mark.parametrize("case", BUILT, ids=lambda c: c.id)
def test_the_case_has_its_stated_property(case):
    if case.prop is not None:
        case.prop(case)
    assert case.n_cus == 1 or case.id == "plain_two_cus"


@pytest.mark.parametrize("case", BUILT, ids=lambda c: c.id)
def test_the_models_image_sweeps_to_brute_force(case):
    win_chunk, rec, carry = case.model_image()
    order = np.random.default_rng(len(case.id)).permutation(len(carry)).tolist()
    got, want = sc.sweep(case, win_chunk, rec, carry, order), sc.brute_force(case)
    assert got == want, [(i, got.get(i), want.get(i)) for i in sorted(set(got) | set(want)) if got.get(i) != want.get(i)][:8]
    if case.id not in ("single_record_paths_64", "single_record_paths_65", "windows_8192"):
        assert any(r for _, r in want.values()), "a case without a revisit does not test the carry"


@pytest.mark.parametrize("case", BUILT, ids=lambda c: c.id)
def test_the_checker_passes_the_models_image(case):
    case.check(case.model_dump())


def wrong(case, edit):
    """The model's dump with `edit` applied to (win_chunk, rec, carry), as bytes."""
    raw = bytearray(case.model_dump())
    d = sc.Dump(bytes(raw))
    at = 88
    win_chunk = np.frombuffer(raw, dtype=np.uint32, count=d.n_win + 1, offset=at)
    rec = np.frombuffer(raw, dtype=np.uint32, count=d.n_chunks * 64, offset=at + 4 * (d.n_win + 1))
    carry = np.frombuffer(raw, dtype=np.uint32, count=d.n_chunks, offset=at + 4 * (d.n_win + 1) + 256 * d.n_chunks)
    edit(win_chunk, rec, carry)
    return bytes(raw)


def case_of(id):
    return next(c for c in sc.CASES if c.id == id)


def edit_carry(win_chunk, rec, carry):
    carry[2] = 445 + 2  # (the largest end of chunk 1 alone)


def edit_ordinal(win_chunk, rec, carry):
    rec[:] = np.where(rec & sc.PAD, rec, rec + (1 << sc.ORD_SHIFT))


def edit_padding(win_chunk, rec, carry):
    rec[rec == sc.PAD] = 0


def edit_flag(win_chunk, rec, carry):
    rec[150] &= ~np.uint32(sc.FIRST)


def edit_start(win_chunk, rec, carry):
    rec[70] += 1


def edit_layout(win_chunk, rec, carry):
    win_chunk[-1] += 1


@pytest.mark.parametrize("edit", [edit_carry, edit_ordinal, edit_padding, edit_flag, edit_start, edit_layout], ids=lambda f: f.__name__)
def test_the_checker_notices_a_wrong_word(edit):
    case = case_of("three_chunks_one_path")
    with pytest.raises(AssertionError):
        case.check(wrong(case, edit))


def test_the_checker_holds_a_refusal_to_its_reason():
    import struct
    case = case_of("memory")
    ok = struct.pack("<8q", 1, -1, -1, 0, 1000, 0, case.n_win, 0) + b"memory".ljust(16, b"\0") + struct.pack("<q", -1)
    case.check(ok)
    for bad in (ok.replace(b"memory", b"errory"), struct.pack("<8q", 1, -1, -1, 4, 1000, 0, case.n_win, 0) + ok[64:]):
        with pytest.raises(AssertionError):
            case.check(bad)
