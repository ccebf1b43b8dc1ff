"""flip at its kernels' seams (tests/flip_shapes.py: tile edges, paths of no or few steps, spans that are not laid out, rows of
the key table at the thresholds between the three sorts, one pair walked 10^5 times, scan tiles), sums past 32 bits, its
refusals, and a stream of the caller's.  Every constant comes from the source text (flip_model.source_constants, which
tests/test_flip_model.py holds to the model's).  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import flip_gpu as fg
import flip_model as fm
import flip_shapes as fs
import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu
T = fs.T
h = fs.h
BOUNDS, TOO_LARGE = -2, -6


def test_the_shapes_straddle_the_sources_constants():
    c = fm.source_constants()
    assert T == c["THREADS"] * c["PER"] and fm.SHORT_ROW == c["SHORT_ROW"] and fm.LDS_ROW == c["LDS_ROW"] and fm.SCAN_TILE == c["THREADS"] * c["SCAN_PER"]


@pytest.fixture(scope="module")
def wants():
    """Per shape: the pools and the model's flip of them, made once for the two routes."""
    return {}


def model_of(wants, name, table):
    if name not in wants:
        p = table[name]()
        wants[name] = (p, fm.flip(p))
    return wants[name]


@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_shape_device_pair(name, wants):
    p, want = model_of(wants, name, fs.SHAPES)
    fg.check_device_pair(p, want, what=name)


@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_shape_handle(name, wants):
    p, want = model_of(wants, name, fs.SHAPES)
    fg.check_handle(p, want, what=name)


@pytest.mark.parametrize("name", list(fs.HEAVY))
def test_sums_past_32_bits(name, wants):
    p, want = model_of(wants, name, fs.HEAVY)
    _, _, turned = fg.check_device_pair(p, want, what=name)
    assert fg.u32(turned).tolist() == [1 if name.startswith("rev") else 0, 1]
    fg.check_handle(p, want, what=name)


def test_one_pair_walked_10_to_the_5_times_adds_one_link(wants):
    p, want = model_of(wants, "one pair 10^5 times", fs.SHAPES)
    _, links_out, _ = fg.check_device_pair(p, want)
    assert fg.u32(links_out).reshape(-1, 4).tolist() == [[h(0), h(1), 0, 1], [h(1), h(1), 1, 2]]


def test_a_stream_of_the_callers(wants):
    import torch
    st = torch.cuda.Stream()
    for name in ("paths of 0, 1 and 2 steps between long ones", "gapped, overlapping and out-of-order spans", "rows of SHORT+1 and SHORT-1 keys"):
        p, want = model_of(wants, name, fs.SHAPES)
        fg.check_device_pair(p, want, stream=st, what=name)


# ---- rounds of the key table ----
ROUND_SHAPES = ["paths of T-1, T, T+1, 2T+1 steps, every other turned", "gapped, overlapping and out-of-order spans", "many whole paths in one tile",
                "paths of 0, 1 and 2 steps between long ones"]


def round_sizes(p):
    """Round sizes at which the key table of p is cut in more than one round -- the smallest that holds its longest row, and
    thirds of the keys and of the candidates, less one, exact and plus one -- with the keys and the upper bound the host has."""
    rows = fm.row_sizes(p)
    longest, keys = max(rows.values()), sum(rows.values())
    cands = keys - len(p.links)
    most = len(p.links) + int((p.paths["steps_end"].astype(np.int64) - p.paths["steps_start"]).sum())
    sizes = {longest} | {n // 3 + d for n in (keys, cands) for d in (-1, 0, 1)}
    return sorted(r for r in sizes if r >= longest and most > 2 * r), keys


@pytest.mark.parametrize("name", ROUND_SHAPES)
def test_the_round_cuts_move_and_the_answer_does_not(name, wants, monkeypatch):
    p, want = model_of(wants, name, fs.SHAPES)
    sizes, keys = round_sizes(p)
    assert len(sizes) >= 4 and keys > 3 * sizes[0]
    dg, links, align = fg.to_device(p)
    for r in sizes:
        new, links_out, turned = pdev.flip(dg, links, alignment=align, round_keys=r)
        assert np.array_equal(fg.u32(new.steps), want.steps) and fg.u32(links_out).tobytes() == want.links.tobytes(), (name, r)
    for r in (sizes[0], sizes[-1]):
        monkeypatch.setenv("FLATGFA_FLIP_ROUND_KEYS", str(r))  # (a test hook: the host route's rounds)
        fg.check_handle(p, want, what=(name, r))


def test_a_row_longer_than_a_round_is_too_large(wants):
    p, want = model_of(wants, "one pair 10^5 times", fs.SHAPES)
    dg, links, align = fg.to_device(p)
    with pytest.raises(pa.FlatGFAError) as e:
        pdev.flip(dg, links, alignment=align, round_keys=1000)
    assert e.value.code == TOO_LARGE and "share one handle" in _lib.last_error()
    new, links_out, _ = pdev.flip(dg, links, alignment=align, round_keys=100000)  # (two rounds' scratch holds all keys: one round)
    assert fg.u32(links_out).tobytes() == want.links.tobytes()


# ---- refusals ----
def small():
    return fs.graph([2, 2, 3], [[h(0), h(1, True)], [h(2, True), h(1, True), h(0)]], [(h(0), h(1), [fs.op(0)]), (h(1), h(2), [fs.op(4)])])


def raw_count(dg, links, align, n_lin, start):
    job = ctypes.c_void_p()
    a, b, c = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = _lib.lib().flatgfa_dev_flip_count(pdev._ptr(dg.steps), dg.n_steps, start.data_ptr(), pdev._ptr(dg.path_begin), dg.n_paths, n_lin, pdev._ptr(dg.seg_len),
                                           dg.n_segs, pdev._ptr(links), links.numel() // 4, pdev._ptr(align), align.numel(), 0, None, ctypes.byref(job),
                                           ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return rc, job, (a.value, b.value, c.value)


def start_of(dg):
    import torch
    s = np.zeros(dg.n_paths + 1, np.uint32)
    s[1:] = np.cumsum(dg.h_path_end.astype(np.int64) - dg.h_path_begin)
    return torch.from_numpy(s.view(np.int32)).to(dg.device), int(s[-1])


BAD = {
    "a step names segment n_segs": (lambda p: p.steps.__setitem__(3, h(3)), "a step refers to a segment id"),
    "a link's from names segment n_segs": (lambda p: p.links.__setitem__(1, (h(3, True), h(0), 1, 2)), "a link refers to a segment id"),
    "a link's to names segment n_segs": (lambda p: p.links.__setitem__(0, (h(0), h(3), 0, 1)), "a link refers to a segment id"),
    "an overlap one past the alignment pool": (lambda p: p.links.__setitem__(1, (h(1), h(2), 1, 3)), "overlap span outside the alignment pool"),
    "an overlap that ends before it begins": (lambda p: p.links.__setitem__(1, (h(1), h(2), 2, 1)), "overlap span outside the alignment pool"),
    "a path one past the steps": (lambda p: p.paths.__setitem__(1, (2, 4, 3, 6, 0, 0)), "step span outside the steps pool"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_the_device_pair_refuses(name):
    p = small()
    dg, links, align = fg.to_device(p)
    start, n_lin = start_of(dg)
    rc, job, totals = raw_count(dg, links, align, n_lin, start)  # (as it stands it is accepted)
    assert rc == 0 and job.value and totals == (1, 4, 2)
    _lib.lib().flatgfa_dev_flip_free(job)
    poke, message = BAD[name]
    poke(p)
    with pytest.raises(IndexError):
        fm.flip(p)
    dg, links, align = fg.to_device(p)
    start, n_lin = start_of(dg)
    rc, job, totals = raw_count(dg, links, align, n_lin, start)
    assert rc == BOUNDS and job.value is None and message in _lib.last_error()


def test_path_starts_that_do_not_add_up_are_refused():
    import torch
    p = small()
    dg, links, align = fg.to_device(p)
    for starts, n_lin in (([0, 2, 4], 5), ([0, 3, 2], 2), ([1, 3, 6], 6), ([0, 2, 5], 4)):
        start = torch.from_numpy(np.array(starts, np.uint32).view(np.int32)).to(dg.device)
        rc, job, _ = raw_count(dg, links, align, n_lin, start)
        assert rc == BOUNDS and job.value is None, starts


TEXT = b"S\t1\tAA\nS\t2\tCC\nS\t3\tGGG\nP\tp0\t1+,2-\t*\nP\tp1\t3-,2-,1+\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t4M\n"  # small(), as text


def poke(g, pool, index, words):
    """Element `index` of a heap handle's pool gets these u32 words, behind the library's back: the loaders refuse a file that
    holds such a link, so this is the one way a handle comes to hold it."""
    data, n, es = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib().flatgfa_pool(g._h, fo.POOL_ORDER.index(pool), ctypes.byref(data), ctypes.byref(n), ctypes.byref(es)) == 0
    assert index < n.value and es.value == 4 * len(words)
    dst = ctypes.cast(data.value + es.value * index, ctypes.POINTER(ctypes.c_uint32))
    for k, w in enumerate(words):
        dst[k] = w


HANDLE_BAD = {
    "a step names segment n_segs": ("steps", 3, [h(3)], "a step refers to a segment id"),
    "a link's to names segment n_segs": ("links", 0, [h(0), h(3), 0, 1], "a link refers to a segment id"),
    "an overlap one past the alignment pool": ("links", 1, [h(1), h(2), 1, 3], "overlap span outside the alignment pool"),
    "a path one past the steps": ("paths", 1, [2, 4, 3, 6, 0, 0], "step span outside the steps pool"),
    "a segment one past seq_data": ("segs", 2, [3, 0, 4, 8, 0, 0], "sequence span outside seq_data"),
}


@pytest.mark.parametrize("name", list(HANDLE_BAD))
def test_the_handle_refuses(name):
    g = pa.parse_bytes(TEXT)
    try:
        for n in ("steps", "paths", "links", "alignment", "segs"):  # (the text is small())
            assert getattr(fm.pools_of(g), n).tobytes() == getattr(small(), n).tobytes()
        assert g.flip_count() == (1, 4)
        pool, index, words, message = HANDLE_BAD[name]
        poke(g, pool, index, words)
        for call in (g.flip, g.flip_count):
            with pytest.raises(pa.FlatGFAError) as e:
                call()
            assert e.value.code == BOUNDS and message in _lib.last_error()
    finally:
        g.close()


def aliased(n_paths, n_links):
    """n_paths paths that all walk the same 2^16 steps (backward, of one segment), and n_links links."""
    lk = [(h(0), h(0), [])] * n_links
    return fs.graph([1], [], lk, spans=[(0, 1 << 16)] * n_paths, steps=np.full(1 << 16, h(0, True), np.uint32))


def test_more_links_and_steps_than_ordinals_is_too_large_before_any_scratch():
    # 65535 paths over the same 65536 steps lay out 2^32 - 2^16 steps; with 2^16 - 1 links that is one more than fits
    p = aliased((1 << 16) - 1, (1 << 16) - 1)
    dg, links, align = fg.to_device(p)
    start, n_lin = start_of(dg)
    assert n_lin + len(p.links) == (1 << 32) - 1
    rc, job, _ = raw_count(dg, links, align, n_lin, start)
    assert rc == TOO_LARGE and job.value is None and "more than 2^32 - 1 links may be kept" in _lib.last_error()


def test_more_laid_out_steps_than_2_to_the_32_is_too_large_on_the_handle():
    p = aliased((1 << 16) + 1, 0)
    with fm.handle_of(p) as g:
        with pytest.raises(pa.FlatGFAError) as e:
            g.flip()
        assert e.value.code == TOO_LARGE and "more than 2^32 - 1 steps" in _lib.last_error()
