"""The device GFA parser where its layout has seams: items, step fields, lines and newlines on the edges of the text tiles
the step kernels work by, long fields across them, name tables of every shape, and more tiles than one tile of the tiled
scan holds.  T is the tile size the library reports, never a number written here.  Every case must take the device route
and give the host parser's pools in both modes.  Run with -m gpu."""
import numpy as np
import pytest

import pollen_amd as pa
import parse_shapes as ps
from test_gpu_parse import check_against_host
from test_host import QUIRKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    with pa.parse_bytes_device(b"S\t1\tA\n") as g:
        assert g.parsed_on == "device" and g.parse_info["tiles"] == 1
        return g.parse_info["tile_bytes"]


def on_device(text):
    for stream in (False, True):
        assert check_against_host(text, stream, "device") == "device"
    return pa.parse_bytes_device(text)


def step_counts(g):
    p = g.pool("paths")
    return (p["steps_end"].astype(np.int64) - p["steps_start"]).tolist()


def test_tiles_are_counted(T):
    for n, tiles in ((T - 7, 1), (T, 1), (T + 1, 2), (3 * T, 3)):
        with on_device(ps.s_block(n)[0]) as g:
            assert g.parse_info["tiles"] == tiles and g.parse_info["tile_bytes"] == T


@pytest.mark.parametrize("k", range(-1, 8))
def test_item_across_a_tile_edge(T, k):
    with on_device(ps.item_on_edge(T, k)) as g:
        assert step_counts(g) == [3]
        assert g.pool("steps").tolist() == [1 << 1, 0 << 1, 1 << 1 | 1]  # 12345 is the first segment, 1 the second


def test_step_field_ends_on_tile_edges(T):
    with on_device(ps.field_begins_on_tile(T)) as g:
        assert step_counts(g) == [3]
    text = ps.field_ends_on_tile(T)
    with on_device(text) as g:
        assert step_counts(g) == [text[:2 * T].rsplit(b"\t", 1)[1].count(b",") + 1, 1]


def test_short_and_long_lines(T):
    with on_device(ps.short_lines_in_one_tile(T)) as g:
        assert step_counts(g) == [2, 0, 1, 3, 1]
    text = ps.line_across_tiles(T)
    with on_device(text) as g:
        assert step_counts(g) == [ps.steps_exact(3 * T).count(b",") + 1, 1]
    with on_device(ps.many_short_paths(1000)) as g:
        assert step_counts(g) == [1 + i % 5 for i in range(1000)]
        starts = g.pool("paths")["steps_start"].tolist()
        assert starts == np.concatenate([[0], np.cumsum([1 + i % 5 for i in range(999)])]).tolist()


def test_newlines_on_tile_edges(T):
    on_device(ps.newline_ends_tile(T)).close()
    on_device(ps.newline_begins_tile(T)).close()
    # ... and an unterminated last line that begins a tile (parse_stream keeps it, parse_mem drops it)
    text = ps.s_block(T)[0] + b"P\tlast\t1+,2-\t*"
    with pa.parse_bytes_device(text, stream=True) as s, pa.parse_bytes_device(text) as m:
        assert (s.path_count, m.path_count) == (1, 0) and s.parsed_on == m.parsed_on == "device"
    on_device(text).close()


def test_long_fields_across_tile_edges(T):
    for text in (ps.one_long_segment(T + 100), ps.one_long_segment(3 * T), ps.long_optional(T + 50), ps.long_cigar(T // 2, T - 50),
                 ps.long_overlaps(T // 4), ps.path_name(T + 10)):
        assert len(text) > T
        on_device(text).close()


def test_names(T):
    for text in (ps.digit_names(), ps.reversed_names(), ps.skipped_names(), ps.duplicate_names(T, True), ps.duplicate_names(T, False)):
        on_device(text).close()
    for k in (9, 10, 11, 12):  # the name quirks of tests/test_host.py are plain
        on_device(QUIRKS[k]).close()


def test_scan_spine(T):
    text = ps.scan_spine(T)
    with pa.parse_bytes_device(text) as g, pa.parse_bytes(text) as h:
        assert g.parsed_on == "device" and g.parse_info["tiles"] > ps.SCAN_TILE
        assert ps.pools_of(g) == ps.pools_of(h)
        counts = step_counts(g)
        assert max(counts) > T // 2 and min(counts) == 1  # a path longer than a tile, one shorter than a lane's 16 bytes
        assert set((g.pool("steps") & 1).tolist()) == {0, 1}
    with pa.parse_bytes_device(text, stream=True) as g, pa.parse_stream_bytes(text) as h:
        assert g.parsed_on == "device" and ps.pools_of(g) == ps.pools_of(h)
