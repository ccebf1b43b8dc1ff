"""FlatGFA.inject (flatgfa_inject, flatgfa_inject_bed, `fgfa inject`) at the geometry shapes of tests/inject_shapes.py, with
links and seq spans of their own: the segment records, the forward links behind every cut, the remapped old links, the name
table and the path records, past an output tile, a block of links and a few names -- every pool, byte for byte, against the
vectorized model that tests/test_inject_shapes.py pins to inject_model.inject(links=True); and two properties that do not
come from the model: every old path spells what it spelled, and new path l spells [lo, hi) of its path.  Run with -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import chop_model as cm
import inject_model as m
import inject_shapes as sh
import pollen_amd as pa
from conftest import ROOT
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from test_gpu_chop_geometry import host_handle

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")

# name: (image, links of its own, seq spans that are not one behind another, also as BED text, also resident)
SHAPES = {
    "cut rows": (sh.cut_rows, 257, True, False, True),
    "257 segments": (lambda: sh.many_segments(257), 0, False, False, False),
    "4097 segments": (lambda: sh.many_segments(4097), 5000, False, False, False),
    "expansion 6143": (lambda: sh.expansion(3 * sh.OUT_TILE - 1), 255, False, False, False),
    "expansion 6144": (lambda: sh.expansion(3 * sh.OUT_TILE), 256, False, False, False),
    "expansion 6145": (lambda: sh.expansion(3 * sh.OUT_TILE + 1), 257, False, False, False),
    "whole tiles backward": (sh.whole_tiles_backward, 256, False, False, False),
    "seam ends": (lambda: sh.seam_ends(2), 255, False, False, False),
    "unsorted, nested": (sh.unsorted_nested, 257, True, True, False),
    "overlapping spans": (sh.overlapping_spans, 5000, False, False, False),
    "1025 lines": (lambda: sh.line_counts(1025), 0, False, False, False),
    "70001 lines on one path": (lambda: sh.many_lines_one_path(70001), 5000, False, True, True),
    "2049 long rows": (lambda: sh.long_rows(2049), 257, False, False, False),
}


def image_of(what) -> sh.Image:
    make, L, scattered = SHAPES[what][:3]
    im = sh.with_links(make(), L, seed=len(what))
    return sh.scattered_spans(im, seed=L) if scattered else im


def list_of(im: sh.Image):
    return [(int(p), int(a), int(b), nm) for p, a, b, nm in zip(im.line_path, im.lo, im.hi, sh.new_names(im))]


@pytest.mark.parametrize("what", list(SHAPES))
def test_every_pool_of_the_handle_route(what):
    bed, resident = SHAPES[what][3:]
    im = image_of(what)
    p = sh.pools_of(im)
    answer = sh.fast(im)
    g = host_handle(p)
    try:
        assert sh.differing(cm.pools_of(g), p) == []  # (the handle holds exactly these pools)
        fasta = g.flatten_fasta(b"x")
        for links in (False, True):
            want = sh.fast_pools(im, links, p, answer)
            assert len(want.links) == ((len(want.segs) - len(p.segs) + len(p.links)) if links else 0)
            q = g.inject(list_of(im), links)
            got = cm.pools_of(q)
            assert sh.differing(got, want) == [], links
            if bed:  # the BED text names the paths and is parsed by the library
                q2 = g.inject(m.bed_text(sh.lines_of(im)), links)
                assert sh.differing(cm.pools_of(q2), want) == [], links
                q2.close()
            if links:
                # not from the model: what the paths spell, and the pieces in segment order
                sh.check_spelling(im, p, got)
                assert q.flatten_fasta(b"x") == fasta
            q.close()
        if resident:
            g.to_device()
            for links in (False, True):
                q = g.inject(list_of(im), links)
                assert sh.differing(cm.pools_of(q), sh.fast_pools(im, links, p, answer)) == [], links
                q.close()
    finally:
        g.close()


def test_cut_rows_through_the_cli_with_links(tmp_path):
    im = image_of("cut rows")
    p = sh.pools_of(im)
    src, bed, out = tmp_path / "in.flatgfa", tmp_path / "lines.bed", tmp_path / "out.flatgfa"
    src.write_bytes(fo.dump_flatgfa(p))
    bed.write_bytes(m.bed_text(sh.lines_of(im)))
    r = subprocess.run([FGFA, "-i", str(src), "-o", str(out), "inject", "-b", str(bed), "-l"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    q = pa.load(str(out))
    try:
        assert sh.differing(cm.pools_of(q), sh.fast_pools(im, True, p)) == []
    finally:
        q.close()


def test_a_ring_stays_a_graph_its_paths_walk():
    im = sh.ring()
    assert len(im.seg_len) == 3000 and len(im.lo) == 5000 and len(im.links) == 3000
    p = sh.pools_of(im)
    g = host_handle(p)
    try:
        assert len(g.validate()) == 0
        q = g.inject(list_of(im), links=True)
        want = sh.fast_pools(im, True, p)
        assert sh.differing(cm.pools_of(q), want) == []
        assert len(want.segs) > 2 * len(p.segs)  # (most segments are cut)
        assert len(q.validate()) == 0  # the old paths over the forward and the remapped links, the new ones over the same
        assert np.array_equal(q.seg_depth().astype(np.uint64), fo.seg_depth_with_uniq(want)[0].astype(np.uint64))
        sh.check_spelling(im, p, cm.pools_of(q))
        q.close()
    finally:
        g.close()


def test_a_link_past_the_segments():
    im = sh.with_links(sh.unsorted_nested(), 300, seed=3)
    S = len(im.seg_len)
    bad = sh.Image(im.seg_len, im.steps, im.path_begin, im.path_end, im.line_path, im.lo, im.hi, None, im.links.copy())
    bad.links[280] = (3, S << 1)  # in the second block of k_check_links
    g = host_handle(sh.pools_of(bad))
    good = host_handle(sh.pools_of(im))
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            g.inject(list_of(im), links=True)
        assert e.value.code == -2 and "a link refers" in _lib.last_error()
        q = good.inject(list_of(im), links=True)  # the next call, on a good handle, is right
        assert sh.differing(cm.pools_of(q), sh.fast_pools(im, True, cm.pools_of(good))) == []
        q.close()
        q = g.inject(list_of(im), links=False)  # without the links, nothing reads the bad one
        assert sh.differing(cm.pools_of(q), sh.fast_pools(bad, False, cm.pools_of(g))) == []
        q.close()
    finally:
        g.close()
        good.close()
