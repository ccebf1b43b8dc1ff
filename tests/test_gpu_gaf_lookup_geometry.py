"""The GAF lookup's kernels on their edges: tile, step and chunk ends, long lines, many lines, huge segments, every alignment.

The units are those of tests/gaf_lookup_shapes.py (64-byte wave steps, 16 KiB line-index tiles, 16 KiB output tiles); the
answers come from tests/gaf_lookup_model.py or from a closed form that tests/test_gaf_lookup_shapes.py pins to it.
"""
import ctypes
import os

import pytest

import gaf_lookup_model as M
import gaf_lookup_shapes as Sh
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TINY_GFA = os.path.join(GOLDEN, "ref_tiny.gfa")
CHUNKS = ("1", "4096", "50000")  # a chunk per line; a chunk below one tile; a few tiles
OUT_BOUNDS = ("7", "16400")      # pieces below a lane's 16 bytes; a piece of an output tile and 16 bytes


def load(text):
    import pollen_amd as pa
    return pa.parse_bytes(text), M.Graph.from_gfa(text)


def tiny():
    return load(open(TINY_GFA, "rb").read())


def check_all(g, mg, text):
    assert g.gaf_seqs(text) == M.seqs_text(mg, text)
    assert g.gaf_table(text) == M.table_text(mg, text)
    assert g.gaf_count(text) == M.count(mg, text)[0]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("out_bound", OUT_BOUNDS)
def test_every_part_of_a_record_across_step_tile_and_chunk_ends(chunk, out_bound, monkeypatch):
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
    monkeypatch.setenv("FLATGFA_GAF_OUT_BYTES", out_bound)
    g, mg = tiny()
    for boundary in (Sh.STEP, Sh.TILE):
        check_all(g, mg, Sh.padded_reads(mg, 21, boundary, span=70))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_long_lines(chunk, monkeypatch):
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
    g, mg = tiny()
    ok = Sh.gaf_line(b"ok", b">1", 0, 1)
    # a path field of over 64 line-index tiles (and so a line longer than every chunk size here)
    n = 64 * Sh.TILE // 2 + 1000
    per = sum(len(s) for s in mg.seqs)
    line = Sh.long_path_line(mg, n, 5, (n // 8) * per + 3)  # (the read ends half way along the path)
    assert line.index(b"\t100\t") - line.index(b"\t>") > 64 * Sh.TILE
    text = ok + line + ok
    assert g.gaf_count(text) == Sh.long_path_count(n) + 2
    want = M.seqs_text(mg, text)
    assert g.gaf_seqs(text) == want
    reads = g.all_reads(text)
    assert [len(r) for r in reads] == [1, n, 1]
    assert reads[1].chunks[n // 2 + 5].range == (1, 0) and reads[1].sequence().encode() == want.split(b"\n")[1].split(b"\t")[1]


def test_no_lines_is_no_error():
    g, _ = tiny()
    text = b"x" * (3 * Sh.TILE + 5)  # not a '\n' in it: bad as a line would be, it is none
    assert g.gaf_seqs(text) == b"" and g.gaf_table(text) == b"" and g.gaf_count(text) == 0 and len(g.all_reads(text)) == 0
    assert g.gaf_seqs(Sh.gaf_line(b"ok", b">1", 0, 1) + b"garbage behind the last newline") == b"ok\tC\n"


def test_a_million_short_lines(monkeypatch):
    g, mg = tiny()
    n = 1_000_000
    text = Sh.many_short_lines(mg.names[0], n)
    assert g.gaf_count(text) == n
    assert g.gaf_seqs(text) == Sh.many_short_lines_seqs(mg.seqs[0], n)
    monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", "3000000")
    monkeypatch.setenv("FLATGFA_GAF_OUT_BYTES", "100000")
    assert g.gaf_seqs(text) == Sh.many_short_lines_seqs(mg.seqs[0], n)
    reads = g.all_reads(text)
    assert len(reads) == n and reads[n - 1].chunks[0].range == (0, 1) and reads[n // 2].name == "r"


@pytest.mark.parametrize("out_bound", (None, "1000003"))
def test_one_read_through_a_segment_of_several_mbp(out_bound, monkeypatch):
    if out_bound:
        monkeypatch.setenv("FLATGFA_GAF_OUT_BYTES", out_bound)
    n = 5_000_000 + 17
    gfa, big = Sh.big_segment_gfa(n)
    import pollen_amd as pa
    g = pa.parse_bytes(gfa)
    got = g.gaf_seqs(Sh.big_segment_reads(n))
    want = Sh.big_segment_seqs(big)  # both orientations; every output tile but the first starts inside an event
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("out_bound", OUT_BOUNDS + (None,))
def test_events_of_zero_bytes_between_output_tiles(out_bound, monkeypatch):
    if out_bound:
        monkeypatch.setenv("FLATGFA_GAF_OUT_BYTES", out_bound)
    g, mg = tiny()
    # 4-byte answers, hundreds of empty events between them: an output tile of 16 KiB spans thousands of lines
    text = Sh.zero_byte_events(mg.names, 300) * 9000
    assert g.gaf_seqs(text) == (b"z\t" + mg.seqs[0][:1] + b"\n") * 9000
    assert g.gaf_count(text) == 301 * 9000


def test_names_in_the_others_table_and_above_2_63():
    names = [1, 2, 9223372036854775809, 77, 18446744073709551615, 5]
    gfa = b"H\tVN:Z:1.0\n" + b"".join(b"S\t%d\t%s\n" % (nm, (b"ACGTN" * (i + 1))[:3 + 2 * i]) for i, nm in enumerate(names))
    g, mg = load(gfa)
    assert mg.names == names
    text = Sh.random_reads(mg, 4, 300) + Sh.gaf_line(b"wrap", b">18446744073709551617<36893488147419103231", 1, 4)  # = >1 <2^64-1
    check_all(g, mg, text)
    assert g.all_reads(text)[300].chunks[1].handle.segment.name == 18446744073709551615


def test_start_and_end_that_wrap_u64():
    g, mg = tiny()
    two64 = 1 << 64
    digits = b"1" + b"0" * 200  # 10^200 mod 2^64 = 0: a run of over three wave steps
    text = (Sh.gaf_line(b"w1", b">1>2", str(two64 + 3).encode(), str(3 * two64 + 12).encode()) +
            Sh.gaf_line(b"w2", b">1>2", digits, b"000000000000000000000000000000000000000000000000000000000000000000000000000000011") +
            Sh.gaf_line(b"w3", b"<4", str(two64 - 1).encode(), str(two64 - 1).encode()))
    check_all(g, mg, text)
    assert [e.range for e in g.all_reads(text)[0]] == [(3, 8), (0, 4)]


def test_text_at_all_16_alignments_through_the_device_entry():
    import torch
    from pollen_amd import _lib
    lib = _lib.lib()
    g, mg = tiny()
    text = Sh.padded_reads(mg, 9, Sh.STEP, span=30) + Sh.random_reads(mg, 2, 100)
    want_s, want = M.seqs_text(mg, text), M.reads(mg, text)
    E, L = sum(len(evs) for _, evs in want), len(want)
    src = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    job = ctypes.c_void_p()
    for shift in range(16):
        buf = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
        base = buf.data_ptr()
        off = (-base) % 16 + shift
        buf[off:off + len(text)] = src.cuda()
        torch.cuda.synchronize()
        nl, ne, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib.flatgfa_dev_gaf_count(g._h, base + off, len(text), 1, None, ctypes.byref(job), ctypes.byref(nl), ctypes.byref(ne),
                                       ctypes.byref(nb))
        assert rc == 0, _lib.last_error()
        assert (nl.value, ne.value, nb.value) == (L, E, len(want_s))
        out = torch.zeros(nb.value + 32, dtype=torch.uint8, device="cuda")
        o_off = (-out.data_ptr()) % 16 + (shift * 7) % 16  # the output at every alignment too
        first = torch.zeros(L + 1, dtype=torch.int64, device="cuda")
        handle = torch.zeros(E, dtype=torch.int32, device="cuda")
        kind = torch.zeros(E, dtype=torch.uint8, device="cuda")
        a = torch.zeros(E, dtype=torch.int64, device="cuda")
        b = torch.zeros(E, dtype=torch.int64, device="cuda")
        rc = lib.flatgfa_dev_gaf_fill(job, first.data_ptr(), None, None, handle.data_ptr(), kind.data_ptr(), a.data_ptr(), b.data_ptr(),
                                      out.data_ptr() + o_off, None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert bytes(out[o_off:o_off + nb.value].cpu().numpy()) == want_s, shift
        assert int(out[:o_off].sum()) == 0 and int(out[o_off + nb.value:].sum()) == 0  # nothing written outside
        flat = [ev for _, evs in want for ev in evs]
        assert handle.cpu().tolist() == [ev[0] for ev in flat] and kind.cpu().tolist() == [ev[1] for ev in flat]
        assert [x & M.U64 for x in a.cpu().tolist()] == [ev[2] for ev in flat] and [x & M.U64 for x in b.cpu().tolist()] == [ev[3] for ev in flat]
        assert first.cpu().tolist()[-1] == E
    lib.flatgfa_dev_gaf_free(job)
