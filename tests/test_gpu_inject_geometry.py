"""inject on the GPU at the smallest shapes at which each kernel of inject_device.hip can go wrong (tests/inject_shapes.py:
tile, grid and row-length edges, 32-bit limits), against the vectorized model that tests/test_inject_shapes.py pins to the
rule-by-rule one.  Through device.inject (the flatgfa_dev_inject_* entries).  Run with -m gpu."""
import ctypes
import threading

import numpy as np
import pytest

import inject_shapes as sh
import pollen_amd as pa
from pollen_amd import _lib
from pollen_amd import device as pdev

pytestmark = pytest.mark.gpu


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def on_device(im: sh.Image):
    import torch
    dev = torch.device("cuda:0")
    dg = pdev.DeviceGraph(im.steps.astype(np.uint32), im.path_begin.astype(np.uint32), im.path_end.astype(np.uint32), len(im.seg_len),
                          im.seg_len.astype(np.uint32))
    ids = torch.from_numpy(im.line_path.astype(np.int32)).to(dev)
    lo = torch.from_numpy(im.lo.astype(np.int64)).to(dev)
    hi = torch.from_numpy(im.hi.astype(np.int64)).to(dev)
    return dg, ids, lo, hi


def check(im: sh.Image, stream=None):
    want = sh.fast(im)
    dg, ids, lo, hi = on_device(im)
    out, sf = pdev.inject(dg, ids, lo, hi, stream=stream)
    assert np.array_equal(u32(sf), want.seg_first)
    assert np.array_equal(u32(out.seg_len), want.seg_len)
    assert np.array_equal(u32(out.path_begin), want.path_begin)
    assert np.array_equal(u32(out.path_end), want.path_end)
    assert np.array_equal(u32(out.steps), want.steps)
    return want


# (511 and 512 lines: the distinct scan over M + 1 = 2 n + 1 elements ends one short of a scan tile and begins the next)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 1023, 1024, 1025, (1 << 20) + 5])
def test_line_counts(n):
    check(sh.line_counts(n))


@pytest.mark.parametrize("k", [1, 2, 5])
def test_line_ends_on_seams_and_path_ends(k):
    check(sh.seam_ends(k))


def test_cut_rows():
    want = check(sh.cut_rows())
    assert (np.diff(want.seg_first) - 1).tolist() == [0, 1, 16, 17, 4097, 1, 2, 1]


def test_long_segment_cut_in_the_middle():
    # a segment of 2^32 - 1 bases cut at 2^31, walked forward and backward; positions past 2^32 along the path
    L = (1 << 32) - 1
    im = sh.image([L, 5], [[0 << 1, (0 << 1) | 1, 1 << 1]], [(0, 1 << 31, L), (0, L + (1 << 31) - 1, 2 * L + 5), (0, 2 * L + 1, 2 * L + 4)])
    want = check(im)
    assert want.seg_len.tolist() == [1 << 31, (1 << 31) - 1, 1, 3, 1]


# (1023 .. 1025: the row scan over S + 1 elements on its tile seam; 524288 and 524289: k_sort_short's second grid-stride round)
@pytest.mark.parametrize("S", [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, sh.MAX_GRID * 256, sh.MAX_GRID * 256 + 1])
def test_many_segments(S):
    check(sh.many_segments(S))


@pytest.mark.parametrize("R", [sh.MAX_GRID, sh.MAX_GRID + 1, 2 * sh.MAX_GRID + 1])
def test_long_rows_past_one_round_of_workgroups(R):
    # row 2048 is the first of k_sort_long's second round, row 4096 the first of its third
    want = check(sh.long_rows(R))
    assert len(want.seg_len) == 18 * R


def test_row_lengths_around_powers_of_two():
    check(sh.row_lengths())


@pytest.mark.parametrize("N", [sh.SCAN_TILE - 2, sh.SCAN_TILE - 1, sh.SCAN_TILE])
def test_pool_steps_at_the_scan_tile(N):
    # pre[N] and noff[N], one past the steps, as the last element of a scan tile and as the first of the next
    check(sh.pool_steps(N))


def test_many_paths_take_the_per_path_route_twice_round():
    check(sh.many_paths_non_tiling())


@pytest.mark.parametrize("total", [sh.OUT_TILE * 3 - 1, sh.OUT_TILE * 3, sh.OUT_TILE * 3 + 1])
def test_expansion_tile_edges(total):
    want = check(sh.expansion(total))
    assert want.path_end[0] == total


def test_one_backward_step_fills_whole_output_tiles():
    check(sh.whole_tiles_backward())


def test_overlapping_spans_take_the_per_path_route():
    check(sh.overlapping_spans())


def test_a_whole_long_path_next_to_short_lines():
    want = check(sh.long_and_short_lines())
    assert want.path_end[-1] == len(want.steps)  # a new path that ends in the last step of the pool


def test_70001_lines_on_one_path():
    check(sh.many_lines_one_path())


def test_unsorted_and_nested_lines():
    check(sh.unsorted_nested())


def test_random_images():
    rng = np.random.default_rng(101)
    for _ in range(25):
        check(sh.random_image(rng, int(rng.integers(1, 400)), int(rng.integers(1, 9)), 700, int(rng.integers(0, 300)), max_len=9))


def test_zero_lines_hold_no_scratch_per_step():
    import torch
    n = 8 << 20
    im = sh.image([3, 4], [(np.arange(n) % 2) << 1], [])
    dg, ids, lo, hi = on_device(im)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.mem_get_info()[0]
    rc, s, steps, p, job = count_only(im, dg, free=False)
    during = torch.cuda.mem_get_info()[0]
    _lib.lib().flatgfa_dev_inject_free(job)
    assert rc == 0 and (s, steps, p) == (2, n, 1)
    assert before - during < 6 * n  # (12 bytes a step would be 96 MB; the scans' tile sums are a sixteenth of a byte a step)
    out, sf = pdev.inject(dg, ids, lo, hi)
    assert np.array_equal(u32(out.steps), im.steps) and u32(sf).tolist() == [0, 1, 2]


def count_only(im, dg=None, free=True):
    import torch
    dg, ids, lo, hi = on_device(im) if dg is None else (dg,) + on_device(im)[1:]
    g = dg.c_struct()
    sf = torch.empty(dg.n_segs + 1, dtype=torch.int32, device=dg.device)
    job = ctypes.c_void_p()
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    rc = _lib.lib().flatgfa_dev_inject_count(ctypes.byref(g), ptr(ids), ptr(lo), ptr(hi), len(im.lo), sf.data_ptr(), None,
                                             ctypes.byref(job), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    if job.value and free:
        _lib.lib().flatgfa_dev_inject_free(job)
    return rc, a.value, b.value, c.value, (job.value if free else job)


def test_limit_is_found_by_the_count():
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    rc, _s, _n, _p, job = count_only(sh.limit(4097))  # 2^20 + 4097 * 2^20 new steps
    assert rc == -6 and not job and "steps" in _lib.last_error()
    assert torch.cuda.mem_get_info()[0] >= before - (64 << 20)  # nothing of 16 GB was allocated
    rc, s, n, p, job = count_only(sh.limit(64))  # fits: counted, not filled
    assert rc == 0 and job and (s, n, p) == (16, 65 << 20, 65)


def test_bad_ids():
    im = sh.unsorted_nested()
    bad = sh.Image(im.seg_len, im.steps, im.path_begin, im.path_end, im.line_path.copy(), im.lo, im.hi)
    bad.line_path[4] = len(im.path_begin)  # a path id >= n_paths
    with pytest.raises(pa.FlatGFAError) as e:
        pdev.inject(*on_device(bad))
    assert e.value.code == -2 and "path id" in _lib.last_error()
    bad = sh.Image(im.seg_len, im.steps.copy(), im.path_begin, im.path_end, im.line_path, im.lo, im.hi)
    bad.steps[500] = len(im.seg_len) << 1  # a step >= S inside a walked span
    with pytest.raises(pa.FlatGFAError) as e:
        pdev.inject(*on_device(bad))
    assert e.value.code == -2 and "step" in _lib.last_error()
    check(im)  # and the next call is right


def test_two_jobs_on_two_streams():
    # a thread per stream, several calls each, so that jobs of the two are in flight together (a call waits for its own stream
    # in the count and in the free): the answers are those of one call after the other
    import torch
    shapes = [sh.many_lines_one_path(20000), sh.cut_rows()]
    wants = [sh.fast(im) for im in shapes]
    inputs = [on_device(im) for im in shapes]
    alone = [pdev.inject(*g) for g in inputs]  # one after the other, on the current stream
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in shapes]
    out, errs = [None, None], []

    def run(k):
        try:
            with torch.cuda.stream(streams[k]):
                out[k] = [pdev.inject(*inputs[k], stream=streams[k]) for _ in range(4)]
        except Exception as e:  # (reported below, on the main thread)
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for want, one, res in zip(wants, alone, out):
        for dg, sf in [one] + res:
            assert np.array_equal(u32(sf), want.seg_first) and np.array_equal(u32(dg.seg_len), want.seg_len)
            assert np.array_equal(u32(dg.steps), want.steps)
            assert np.array_equal(u32(dg.path_begin), want.path_begin) and np.array_equal(u32(dg.path_end), want.path_end)
