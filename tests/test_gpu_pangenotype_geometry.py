"""The pangenotype kernels (pollen_amd/csrc/gaf_device.hip) at the geometry they were built for, against matrix_fast of
tests/gaf_model.py: lines longer than a tile and than a lookback batch, tabs tiles apart, '#' lines far from their tokens,
names across tile edges, error lines MBs long in chunked files (tests/gaf_shapes.py); a name table of a million segments;
the device entry at every alignment; a resident graph.  Run with -m gpu."""
import re

import numpy as np
import pytest

import gaf_model as gm
import gaf_shapes as gs
import pollen_amd as pa

pytestmark = pytest.mark.gpu
TILE = gs.GPU_TILE
SEED = 5
CHUNKS = [None, "4096", "100000"]
CHUNK_IDS = ["default_chunks", "4k_chunks", "100k_chunks"]


def error_of(e):
    """(file, offset) of a FlatGFAError from a bad GAF line."""
    assert e.code == -2, str(e)
    m = re.search(r"GAF file (\d+): the line at byte offset (\d+) ", str(e))
    assert m, str(e)
    return int(m.group(1)), int(m.group(2))


def model(texts, names=gs.NAMES):
    """(bool matrix, None) or (None, (file, offset))."""
    try:
        return np.array(gm.matrix_fast(texts, names), dtype=bool).reshape(len(texts), len(names)), None
    except gm.GafError as e:
        return None, (e.file, e.offset)


def run(g, texts):
    try:
        return g.pangenotype_matrix(texts), None
    except pa.FlatGFAError as e:
        return None, error_of(e)


def table_of(m):
    return b"".join(b"".join(b"1" if c else b"0" for c in r) + b"\n" for r in m.tolist())


@pytest.fixture(scope="module")
def shapes_gfa(tmp_path_factory):
    p = tmp_path_factory.mktemp("gaf_geometry") / "shapes.gfa"
    p.write_bytes(gs.gfa())
    return str(p)


@pytest.fixture(scope="module")
def graph(shapes_gfa):
    g = pa.parse(shapes_gfa)
    yield g
    g.close()


@pytest.fixture(scope="module")
def good():
    """Every good shape as a file of its own, then all of them in one file in shuffled order, then an empty file."""
    shapes = gs.good_shapes(TILE, SEED)
    labels = [label for label, _ in shapes]
    texts = [sh.text for _, sh in shapes]
    order = np.random.default_rng(SEED).permutation(len(texts))
    texts += [b"".join(texts[int(i)] for i in order), b""]
    labels += ["shuffled", "empty"]
    want, err = model(texts)
    assert err is None
    for (label, sh), row in zip(shapes, want):
        got = {n for n, b in zip(gs.NAMES, row) if b}
        assert sh.sets <= got and (not sh.exact or got == sh.sets), label
    return labels, texts, want


@pytest.fixture(scope="module")
def bad():
    return gs.bad_shapes(TILE, SEED)


@pytest.mark.parametrize("chunk", CHUNKS, ids=CHUNK_IDS)
def test_shapes_match_model(graph, good, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
    labels, texts, want = good
    wrong = []  # every shape alone first, so that one that errs does not hide the rows of the others
    for label, text, w_row in zip(labels, texts, want):
        got, err = run(graph, [text])
        if err is not None or not (got[0] == w_row).all():
            wrong.append((label, err if err else [gs.NAMES[i] for i in np.flatnonzero(got[0] != w_row)]))
    assert not wrong
    got = graph.pangenotype_matrix(texts)
    assert got.shape == want.shape and (got == want).all()
    assert graph.pangenotype_table(texts) == table_of(want)


@pytest.mark.parametrize("chunk", CHUNKS, ids=CHUNK_IDS)
def test_error_far_into_a_long_line(graph, good, bad, chunk, monkeypatch):
    # the first bad line's offset in its file, whatever piece its bad name and the later bad lines fall into
    if chunk:
        monkeypatch.setenv("FLATGFA_GAF_CHUNK_BYTES", chunk)
    a = good[1][0]
    for label, sh in bad:
        for texts, where in (([sh.text], 0), ([a, b"", sh.text, a], 2), ([sh.text + a], 0)):
            want = model(texts)[1]
            assert want == (where, sh.bad), label
            assert run(graph, texts)[1] == want, (label, where)
        with pytest.raises(pa.FlatGFAError) as e:
            graph.pangenotype_table([a, sh.text])
        assert error_of(e.value) == (1, sh.bad)


@pytest.fixture(scope="module")
def big_table(tmp_path_factory):
    """About a million segments: names 1..k, then a seeded permutation of random u64 names (half of them 2^63 and above,
    2^64 - 1 among them), duplicates of some of those and of sequential names, and one segment named 0."""
    rng = np.random.default_rng(2026)
    k = 300_000
    rand = rng.integers(k + 1, 2**64, size=690_000, dtype=np.uint64, endpoint=False)
    dups = np.concatenate([rng.choice(rand, 5_000), rng.integers(1, k + 1, size=2_000).astype(np.uint64)])
    edge = np.array([2**64 - 1, 2**63, 2**63 - 1, k + 2, 0], dtype=np.uint64)
    others = rng.permutation(np.concatenate([rand, dups, edge]))
    names = list(range(1, k + 1)) + [int(x) for x in others]
    p = tmp_path_factory.mktemp("gaf_names") / "million.gfa"
    p.write_bytes(b"".join(b"S\t%d\tA\n" % n for n in names))
    g = pa.parse(str(p))
    assert g.segment_count == len(names)
    yield g, names
    g.close()


def test_name_table_of_a_million_segments(big_table):
    g, names = big_table
    seq_max, others = gm.name_map(names)
    assert seq_max == 300_000 and len(others) > 600_000 and max(others) == 2**64 - 1 and 0 in others
    rng = np.random.default_rng(7)
    # every name but 0, both copies of each duplicate, in random order, with and without leading zeros
    toks = [(b"<0%d" if i % 3 == 0 else b">%d") % n for i, n in enumerate(names) if n]
    order = rng.permutation(len(toks))
    lines = [b"r%d\t1\t0\t1\t+\t" % j + b"".join(toks[int(i)] for i in order[j:j + 1000]) + b"\t60\n"
             for j in range(0, len(toks), 1000)]
    text = b"".join(lines)
    want, err = model([text], names)
    assert err is None
    # (earlier copies of a duplicate, later copies of a sequential name and segment "0" are never set)
    assert want.sum() == len({gm.lookup((seq_max, others), n) for n in names if n}) < len(names) - 5_000
    got = g.pangenotype_matrix([text])
    assert (got == want).all(), np.flatnonzero(got[0] != want[0])[:20]
    # one bad line each, after a good one: a present key +-1, between seq_max and the smallest other, 0 and what wraps to it
    keys = sorted(x for x in others if x > seq_max)
    present = set(names)
    cands = [keys[0] + 1, keys[1] - 1, keys[1] + 1, 2**63 + 1, 2**63 - 2, 2**64 - 2, keys[len(keys) // 2] + 1, keys[-2] - 1,
             seq_max + 1, keys[0] - 1]
    misses = sorted({c for c in cands if c > seq_max and c not in present})
    assert len(misses) >= 5 and seq_max + 1 in misses
    head = lines[0]
    for name in misses + [0, 2**64]:
        t = head + b"bad\t1\t0\t1\t+\t>1>%d<2\t60\n" % name + head
        assert model([t], names)[1] == (0, len(head)), name
        assert run(g, [t])[1] == (0, len(head)), name


def test_resident_graph_gives_the_same_matrix(shapes_gfa, good, bad):
    _, texts, want = good
    g = pa.parse(shapes_gfa)
    try:
        g.to_device()
        got = g.pangenotype_matrix(texts)
        assert (got == want).all()
        sh = bad[0][1]
        assert run(g, [texts[0], sh.text])[1] == (1, sh.bad)
    finally:
        g.close()


def _bits(row, S):
    return np.unpackbits(row.cpu().numpy().view(np.uint8), bitorder="little")[:S].astype(bool)


def test_device_entry_at_every_alignment(graph, good, bad):
    torch = pytest.importorskip("torch")
    from pollen_amd import device as pdev
    dev = torch.device("cuda:0")
    S, W = len(gs.NAMES), (len(gs.NAMES) + 63) // 64
    labels, texts, _ = good
    cases = [(label, texts[labels.index(label)]) for label in ("A", "D#_first_far", "D_far")]
    cases += [(label, sh.text) for label, sh in bad]
    junk = b"\n\t>0#<976\t\t"  # bytes that would matter, before the text and (without its '\n') behind it
    runs = []
    for label, text in cases:
        want, err = model([text])
        for o in range(16):
            n = len(text) + (0, 1, 7, 15, 16, 33)[o % 6]
            host = (junk * 2)[:o] + text + (junk.replace(b"\n", b"") * 5)[:n - len(text)]
            buf = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
            view = buf[o:o + n]
            assert view.data_ptr() % 16 == o
            row = torch.zeros(W, dtype=torch.int64, device=dev)
            first_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
            pdev.pangenotype_row(graph, view, row, first_bad)
            runs.append((label, o, want, err, buf, row, first_bad))
    # a tail of more than three tiles of tabs and unknown names behind the last '\n'
    text = texts[labels.index("D_first_far")]
    tail = (b"\t>976<0\t>5001" * (3 * TILE // 10 + 100))
    assert len(tail) > 3 * TILE and b"\n" not in tail
    buf = torch.frombuffer(bytearray(text + tail), dtype=torch.uint8).to(dev)
    row = torch.zeros(W, dtype=torch.int64, device=dev)
    first_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
    pdev.pangenotype_row(graph, buf, row, first_bad)
    want, err = model([text])
    runs.append(("long_tail", 0, want, err, buf, row, first_bad))
    torch.cuda.synchronize()
    wrong = []
    for label, o, want, err, _, row, first_bad in runs:
        if int(first_bad.item()) != (-1 if err is None else err[1]) or (err is None and not (_bits(row, S) == want[0]).all()):
            wrong.append((label, o))
    assert not wrong


def test_device_entry_on_two_streams_with_growing_texts(graph, good):
    # every call that outgrows the handle's scratch replaces it (after the last call on any stream); the others wait for
    # that call on the stream they run on
    torch = pytest.importorskip("torch")
    from pollen_amd import device as pdev
    dev = torch.device("cuda:0")
    S, W = len(gs.NAMES), (len(gs.NAMES) + 63) // 64
    labels, texts, _ = good
    mixed = texts[labels.index("shuffled")]
    lengths = [1_000, 50_000, 700_000, 3_000_000, 9_000_000, 20_000_000, len(mixed), 2_000_000, 100]
    bufs = [torch.frombuffer(bytearray(mixed[:n]), dtype=torch.uint8).to(dev) for n in lengths]
    rows = [torch.zeros(W, dtype=torch.int64, device=dev) for _ in lengths]
    bads = [torch.full((1,), -1, dtype=torch.int64, device=dev) for _ in lengths]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for i, buf in enumerate(bufs):
        pdev.pangenotype_row(graph, buf, rows[i], bads[i], stream=streams[i % 2])
    torch.cuda.synchronize()
    for n, row, first_bad in zip(lengths, rows, bads):
        want, err = model([mixed[:n]])
        assert err is None
        assert (_bits(row, S) == want[0]).all(), n
        assert int(first_bad.item()) == -1, n
