"""The pangenotype matrix on the GPU (flatgfa_pangenotype_matrix / _table / flatgfa_dev_pangenotype_row, `fgfa matrix`,
FlatGFA.pangenotype_matrix) against the model in tests/gaf_model.py and the reference's known answer.  Run with -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import gaf_model as gm
import pollen_amd as pa
from conftest import GOLDEN, ROOT, fixture_id, golden_gfas

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")
GAF = os.path.join(GOLDEN, "gaf")
TINY_GFA = os.path.join(GOLDEN, "ref_tiny.gfa")


def gaf(name):
    return os.path.join(GAF, name)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_known_answer_cli():
    for name, want in (("tiny.gaf", b"1111\n"), ("tiny2.gaf", b"1101\n")):
        out = subprocess.run([FGFA, "-I", TINY_GFA, "matrix", gaf(name)], capture_output=True, check=True, timeout=120).stdout
        assert out == want


def test_known_answer_python_and_abi():
    g = pa.parse(TINY_GFA)
    files = [gaf("tiny.gaf"), gaf("tiny2.gaf")]
    assert g.make_pangenotype_matrix(files) == [[True, True, True, True], [True, True, False, True]]  # test_matrix.py:11-18
    assert g.pangenotype_table(files) == b"1111\n1101\n"
    assert g.pangenotype_matrix([read(f) for f in files]).tolist() == [[True] * 4, [True, True, False, True]]


def test_cli_argument_shapes():
    for args in ([], [gaf("tiny.gaf"), gaf("tiny2.gaf")]):
        r = subprocess.run([FGFA, "-I", TINY_GFA, "matrix"] + args, capture_output=True, timeout=120)
        assert r.returncode == 2 and r.stdout == b"" and b"usage" in r.stderr
    r = subprocess.run([FGFA, "-I", TINY_GFA, "matrix", gaf("no_such.gaf")], capture_output=True, timeout=120)
    assert r.returncode != 0 and r.stdout == b""


def seg_names(g):
    return [int(x) for x in g.pool("segs")["name"]]


def synthetic_gaf(g, seed, n_reads=400, long_line=0):
    """Random sub-walks of the graph's paths as >name/<name path fields, among the edge lines of edges.gaf (all but its last
    line, which lacks its '\\n'), and, with `long_line`, one line whose path field is that many bytes long."""
    rng = np.random.default_rng(seed)
    names = seg_names(g)
    steps = g.pool("steps")
    paths = g.pool("paths")
    edges = read(gaf("edges.gaf"))
    edge_lines = [ln + b"\n" for ln in edges[:edges.rindex(b"\n")].split(b"\n")]
    # (their names are ref_tiny's: struck out where they would be read, kept in the '#' line and the 7th column)
    keep = (b"#", b"empty_field")
    edge_lines = [ln if ln.startswith(keep) else ln.replace(b">18446744073709551617", b"").replace(b">0004", b"")
                  .replace(b">1", b"").replace(b">2", b"").replace(b"<2", b"").replace(b">3", b"") for ln in edge_lines]
    out = []
    for r in range(n_reads):
        k = int(rng.integers(0, 10))
        if k == 0:
            # edge lines whose names are not read (skipped lines, other columns) or that name nothing
            out.append(edge_lines[int(rng.integers(0, len(edge_lines)))])
            continue
        field = b""
        if len(paths):
            p = paths[int(rng.integers(0, len(paths)))]
            b, e = int(p["steps_start"]), int(p["steps_end"])
            if e > b:
                i = int(rng.integers(b, e))
                j = int(rng.integers(i, min(e, i + 20)))
                toks = []
                for h in steps[i:j + 1]:
                    h = int(h)
                    pre = b"<" if h & 1 else b">"
                    toks.append(pre + (b"0" * int(rng.integers(0, 2))) + str(names[h >> 1]).encode())
                sep = [b"", b"", b"x"][int(rng.integers(0, 3))]
                field = sep.join(toks)
        tags = b"\t" + b"\t".join(str(int(v)).encode() for v in rng.integers(0, 1000, 6)) + b"\tcg:Z:150M"
        end = b"\r\n" if k == 1 else b"\n"
        out.append(b"read%d\t150\t0\t150\t+\t" % r + field + tags + end)
    if long_line and len(names):
        reps = long_line // (len(str(names[-1])) + 1) + 1
        field = (b">" + str(names[-1]).encode()) * reps
        out.insert(len(out) // 2, b"long\t1\t0\t1\t+\t" + field + b"\t1\t0\n")
    return b"".join(out)


def parsable_goldens():
    out = []
    for path in golden_gfas():
        try:
            pa.parse(path).close()
        except pa.FlatGFAError:
            continue
        out.append(path)
    return out


@pytest.mark.parametrize("chunk", [None, "4096"], ids=["default_chunks", "4k_chunks"])
def test_synthetic_gaf_matches_model_on_every_golden(chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
    graphs = parsable_goldens()
    assert any(fixture_id(p) == "edge_names_loops" for p in graphs)
    for k, path in enumerate(graphs):
        g = pa.parse(path)
        names = seg_names(g)
        texts = [synthetic_gaf(g, 100 + k, long_line=3 * 4096 + 17 if chunk else 0), synthetic_gaf(g, 200 + k, n_reads=40)]
        want = gm.matrix(texts, names)
        got = g.pangenotype_matrix(texts)
        assert got.shape == (2, len(names))
        assert got.tolist() == want, fixture_id(path)
        assert g.pangenotype_table(texts) == gm.table(texts, names), fixture_id(path)
        g.close()


def test_chunk_boundaries_everywhere(monkeypatch):
    # every line straddles some chunk end as the chunk size walks through a line's length
    g = pa.parse(os.path.join(GOLDEN, "edge_names_loops.gfa"))
    names = seg_names(g)
    text = synthetic_gaf(g, 7, n_reads=120, long_line=9000)
    want = gm.matrix([text], names)
    for chunk in (1, 16, 100, 333, 4096):
        monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", str(chunk))
        assert g.pangenotype_matrix([text]).tolist() == want, chunk
    g.close()


@pytest.mark.parametrize("bad", [b">", b">1>77", b">18446744073709551616"], ids=["no_digits", "unknown_name", "wraps_to_zero"])
def test_errors(bad, tmp_path):
    g = pa.parse(TINY_GFA)
    good = read(gaf("tiny.gaf"))
    text = good + b"read\t1\t0\t1\t+\t" + bad + b"\t1\n" + good + b"read\t1\t0\t1\t+\t>9\n"
    with pytest.raises(pa.FlatGFAError) as e:
        g.pangenotype_matrix([good, text])
    assert e.value.code == -2
    msg = str(e.value)
    assert "GAF file 1" in msg and f"byte offset {len(good)} " in msg, msg
    with pytest.raises(gm.GafError) as me:
        gm.matrix([good, text], [1, 2, 3, 4])
    assert (me.value.file, me.value.offset) == (1, len(good))
    f = tmp_path / "bad.gaf"
    f.write_bytes(text)
    r = subprocess.run([FGFA, "-I", TINY_GFA, "matrix", str(f)], capture_output=True, timeout=120)
    assert r.returncode != 0 and r.stdout == b"" and b"byte offset" in r.stderr
    g.close()


def test_several_files_in_one_call(tmp_path):
    g = pa.parse(TINY_GFA)
    empty = tmp_path / "empty.gaf"
    empty.write_bytes(b"")
    no_nl = tmp_path / "no_nl.gaf"
    no_nl.write_bytes(read(gaf("tiny2.gaf")) + b"read\t1\t0\t1\t+\t>3\t1")
    files = [str(empty), gaf("tiny2.gaf"), gaf("tiny2.gaf"), str(no_nl), gaf("edges.gaf")]
    want = gm.matrix([read(f) for f in files], [1, 2, 3, 4])
    assert want[0] == [False] * 4 and want[3] == [True, True, False, True]
    assert g.make_pangenotype_matrix(files) == want
    assert g.pangenotype_table(files) == gm.table([read(f) for f in files], [1, 2, 3, 4])
    r = subprocess.run([FGFA, "-I", TINY_GFA, "matrix", str(empty)], capture_output=True, check=True, timeout=120)
    assert r.stdout == b"0000\n"
    g.close()


def test_not_resident_graph_stays_off_the_device():
    g = pa.synth(1, 10_000, 100, 10_000, "pangenome", False)
    text = b"".join(b"r\t1\t0\t1\t+\t>%d<%d\t1\n" % (i + 1, 10_000 - i) for i in range(100))
    row = g.pangenotype_matrix([text])[0]
    assert row.sum() == 200 and row[:100].all() and row[-100:].all()
    with pytest.raises(pa.FlatGFAError):
        g.residency_ms()  # the step pool was not uploaded
    g.close()


def test_device_entry_on_torch_tensors():
    torch = pytest.importorskip("torch")
    from pollen_amd import device as pdev
    g = pa.parse(os.path.join(GOLDEN, "edge_names_loops.gfa"))
    names = seg_names(g)
    S, W = len(names), (len(names) + 63) // 64
    a, b = synthetic_gaf(g, 31, n_reads=30), synthetic_gaf(g, 32, n_reads=30)
    want = np.array(gm.matrix([a + b], names)[0])
    dev = torch.device("cuda:0")
    row = torch.zeros(W, dtype=torch.int64, device=dev)
    bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
    for piece in (a, b + b"read\t1\t0\t1\t+\t>999"):  # (the tail after the last newline is ignored)
        t = torch.frombuffer(bytearray(piece), dtype=torch.uint8).to(dev)
        pdev.pangenotype_row(g, t, row, bad)
    torch.cuda.synchronize()
    got = np.unpackbits(row.cpu().numpy().view(np.uint8), bitorder="little")[:S].astype(bool)
    assert (got == want).all()
    assert int(bad.item()) == -1  # untouched on good text
    # an unaligned view of a buffer, and an error: the offset is the line's, within the text given
    buf = torch.frombuffer(bytearray(b"xyz" + a + b"r\t1\t0\t1\t+\t>123456\n"), dtype=torch.uint8).to(dev)
    pdev.pangenotype_row(g, buf[3:], row, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == len(a)
    g.close()


def test_scale_million_segments_quarter_gigabyte():
    S = 1 << 20
    g = pa.synth(5, S, 4, 1000, "uniform", False)
    names = np.asarray(g.pool("segs")["name"], dtype=np.uint64)
    assert len(names) == S and len(np.unique(names)) == S
    rng = np.random.default_rng(11)
    toks = 12
    head = np.frombuffer(b"read\t150\t0\t150\t+\t", dtype=np.uint8)
    tail = np.frombuffer(b"\t1000\t100\t250\t150\t150\t60\tcg:Z:150M\n", dtype=np.uint8)
    width = len(head) + toks * 9 + len(tail)
    n_lines = (256 << 20) // width + 1
    ids = rng.integers(0, S // 2, size=(n_lines, toks), dtype=np.int64) * 2  # even ids only: half the row stays clear
    lines = np.empty((n_lines, width), dtype=np.uint8)
    lines[:, :len(head)] = head
    lines[:, -len(tail):] = tail
    tok = lines[:, len(head):len(head) + toks * 9].reshape(n_lines, toks, 9)
    tok[:, :, 0] = np.where(rng.random((n_lines, toks)) < 0.5, ord(">"), ord("<"))
    v = names[ids]
    for d in range(8, 0, -1):  # eight digits, leading zeros
        tok[:, :, d] = (v % 10).astype(np.uint8) + ord("0")
        v = v // 10
    text = lines.tobytes()
    assert len(text) >= 256 << 20
    want = np.zeros(S, dtype=bool)
    want[ids.ravel()] = True
    got = g.pangenotype_matrix([text])[0]
    assert (got == want).all()
    g.close()
