"""The GPU flatten at the edges of its tiles, pieces, chunks and scans (tests/flatten_shapes.py), every shape against
tests/flatten_model.py byte for byte.  Run with -m gpu."""
import ctypes

import pytest

import flatten_model as fm
import flatten_shapes as fs
import pollen_amd as pa
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib

pytestmark = pytest.mark.gpu


def load(p: fo.Pools, tmp_path):
    f = tmp_path / "shape.flatgfa"
    f.write_bytes(fo.dump_flatgfa(p))
    return pa.load(str(f))


@pytest.mark.parametrize("name", list(fs.CATALOG))
def test_shape(name, tmp_path, monkeypatch):
    s = fs.CATALOG[name]()
    if s.chunk is not None:
        monkeypatch.setenv("FLATGFA_FLATTEN_CHUNK_LINES", str(s.chunk))
    p = s.pools
    with load(p, tmp_path) as g:
        assert g.flatten_legend().tolist() == fm.legend(p)
        want = fm.bed(p, s.nm)
        got = g.flatten_bed(s.nm)
        assert len(got) == len(want) and got == want
        if s.fasta:
            want = fm.fasta(p, s.nm)
            got = g.flatten_fasta(s.nm)
            assert len(got) == len(want) and got == want
        if s.chunk is not None:
            # the sink sees the chunks: the header line, then at least a piece per chunk
            sizes = []
            g.flatten_stream(s.nm, 2, lambda b: sizes.append(len(b)))
            assert len(sizes) >= 1 + s.chunks and sum(sizes) == len(fm.bed(p, s.nm))


def test_bad_handle_delivers_nothing(tmp_path):
    p = fs.bad_handle()
    with load(p, tmp_path) as g:
        for what in (2, 3):
            calls = []
            with pytest.raises(pa.FlatGFAError) as e:
                g.flatten_stream(b"x", what, calls.append)
            assert e.value.code == -2 and calls == []
            assert "out of range" in _lib.last_error()
        with pytest.raises(pa.FlatGFAError) as e:
            g.flatten_bed(b"x")
        assert e.value.code == -2
        # the FASTA reads no step
        assert g.flatten_fasta(b"x") == fm.fasta(p, b"x")
