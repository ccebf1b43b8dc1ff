"""The device GFA parser (pa.parse_bytes_device / parse_device, `fgfa -D`) against the host parser on the same text, pool by
pool and byte for byte, in both modes (parse_mem and parse_stream).  tests/test_host.py pins the host parser to the reference.
Texts of the plain grammar (tests/parse_shapes.py: reason) must take the device route -- a condition, not a hope -- and every
other text must give what the host parser gives, handle or error, by the host route with the expected reason.  Run with -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import pollen_amd as pa
import parse_shapes as ps
from conftest import ROOT, golden_gfas
from oracle import flatgfa_oracle as fo
from pollen_amd import _lib
from test_gpu_print import MAKERS, graph_text
from test_host import QUIRKS

pytestmark = pytest.mark.gpu
FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def host_parse(text, stream):
    """The host route's handle, or its error sentence."""
    try:
        return (pa.parse_stream_bytes if stream else pa.parse_bytes)(text), None
    except pa.FlatGFAError:
        return None, _lib.last_error()


def device_parse(text, stream):
    try:
        return pa.parse_bytes_device(text, stream), None
    except pa.FlatGFAError:
        return None, _lib.last_error()


def check_against_host(text, stream, route=None):
    """Same outcome as the host parser; the route and the reason as the grammar says.  Returns the route taken."""
    want, want_err = host_parse(text, stream)
    got, got_err = device_parse(text, stream)
    info = pa.parse_device_info()
    why = ps.reason(text, stream)
    assert info["reason"] == why, (why, info)
    assert info["parsed_on"] == ("device" if why == "plain" else "host")
    if route is not None:
        assert info["parsed_on"] == route
    if want is None:
        assert got is None and got_err == want_err
        assert why != "plain"
        return "error"
    assert got is not None, got_err
    assert got.parsed_on == info["parsed_on"] and got.parse_reason == why
    for name in fo.POOL_ORDER:
        assert got.pool(name).tobytes() == want.pool(name).tobytes(), (name, stream)
    return info["parsed_on"]


def check_cli(text, tmp_path):
    """`fgfa -D -I FILE -o X` and `fgfa -D -o X` on stdin write the files the host route writes."""
    src = tmp_path / "in.gfa"
    src.write_bytes(text)
    run = lambda *a, **k: subprocess.run([FGFA, *a], capture_output=True, timeout=120, **k)
    for args, kw in ((["-I", str(src)], {}), ([], {"input": text})):
        host, dev = str(tmp_path / "host.flatgfa"), str(tmp_path / "dev.flatgfa")
        r = run(*args, "-o", host, **kw)
        assert r.returncode == 0, r.stderr
        r = run("-D", *args, "-o", dev, **kw)
        assert r.returncode == 0, r.stderr
        assert read(dev) == read(host)


@pytest.mark.parametrize("gfa", ps.all_golden_gfas(), ids=ps.golden_id)
def test_golden(gfa, tmp_path):
    text = read(gfa)
    for stream in (False, True):
        assert check_against_host(text, stream, "device") == "device"
    with pa.parse_device(gfa) as g, pa.parse(gfa) as h:
        assert g.parsed_on == "device" and ps.pools_of(g) == ps.pools_of(h)
    check_cli(text, tmp_path)


@pytest.mark.parametrize("name", list(ps.HANDMADE))
def test_handmade(name, tmp_path):
    for stream in (False, True):
        assert check_against_host(ps.HANDMADE[name], stream, "device") == "device"
    check_cli(ps.HANDMADE[name], tmp_path)


def test_the_new_graph_answers_like_any_other():
    with pa.parse_bytes_device(ps.HANDMADE["plain"]) as g, pa.parse_bytes(ps.HANDMADE["plain"]) as h:
        assert g.parsed_on == "device"
        assert g.gfa_text() == h.gfa_text() == ps.HANDMADE["plain"]
        assert g.depth_table() == h.depth_table()


@pytest.mark.parametrize("k", range(len(QUIRKS) + len(ps.ADDED)))
def test_quirks(k):
    text = (QUIRKS + ps.ADDED)[k]
    table, i = (ps.QUIRKS_NOT_PLAIN, k) if k < len(QUIRKS) else (ps.ADDED_NOT_PLAIN, k - len(QUIRKS))
    assert ps.reason(text) == table.get(i, "plain")
    for stream in (False, True):
        route = check_against_host(text, stream)
        if not ps.plain(text, stream):
            assert route in ("host", "error")


def test_window_of_digits():
    """Numbers of 32 digits are the device's; of 33, the host parser's."""
    for digits, route in ((32, "device"), (33, "host")):
        name = b"0" * (digits - 1) + b"7"
        text = b"S\t" + name + b"\tAC\nS\t2\tG\nL\t" + name + b"\t+\t2\t-\t" + b"0" * (digits - 2) + b"12M\nP\tp\t" + name + b"+,2-," + name + b"-\t*\n"
        for stream in (False, True):
            assert check_against_host(text, stream, route) == route


def test_differential_fuzz():
    """The mutation scheme of tests/test_host.py's test_parser_differential_fuzz: one to three byte edits of a golden text."""
    rng = np.random.default_rng(20240)
    alphabet = np.frombuffer(b"\t\n+-,*0123456789SPLHMACGTx", dtype="u1")
    count = {"device": 0, "host": 0, "error": 0}
    k = 0
    for gfa in golden_gfas():
        base = np.frombuffer(read(gfa), dtype="u1")
        for _ in range(200):  # (host-route successes are the rare class: about one mutant in forty)
            buf = base.copy()
            for _k in range(int(rng.integers(1, 4))):
                op = int(rng.integers(0, 3))
                pos = int(rng.integers(0, len(buf)))
                if op == 0:
                    buf[pos] = alphabet[int(rng.integers(0, len(alphabet)))]
                elif op == 1:
                    buf = np.delete(buf, pos)
                else:
                    buf = np.insert(buf, pos, alphabet[int(rng.integers(0, len(alphabet)))])
            k += 1
            count[check_against_host(buf.tobytes(), k % 2 == 1)] += 1
    print(count)
    assert count["device"] > 50 and count["host"] > 50 and count["error"] > 50, count


@pytest.mark.parametrize("what", list(MAKERS))
def test_round_trip_of_the_other_features(what):
    """What chop, crush, inject and extract make, printed on the device and parsed there again: the printed graph's pools
    but for the line order, which a normalized graph does not have and a parsed text does."""
    make, _args = MAKERS[what]
    with pa.parse_bytes(graph_text()) as g, make(g) as q:
        text = q.gfa_text_device()
        assert ps.plain(text)
        assert check_against_host(text, False, "device") == "device"
        with pa.parse_bytes_device(text) as back:
            assert back.parsed_on == "device"
            assert ps.normalized_pools(back) == ps.normalized_pools(q)
            assert back.gfa_text() == text


def test_limit_branch(monkeypatch):
    """The item limit lowered below a text's step count: the host route, for "limit", and the same pools."""
    text = b"S\t1\tA\nS\t2\tC\nP\tp\t1+,2-,1+,2+,1-,2-,1+\t*\n"  # seven steps; no other pool has more than three items
    monkeypatch.setenv("FLATGFA_PARSE_DEVICE_LIMIT", "6")
    with pa.parse_bytes_device(text) as g, pa.parse_bytes(text) as h:
        assert (g.parsed_on, g.parse_reason) == ("host", "limit")
        assert ps.pools_of(g) == ps.pools_of(h)
    monkeypatch.setenv("FLATGFA_PARSE_DEVICE_LIMIT", "100")
    with pa.parse_bytes_device(text) as g:
        assert (g.parsed_on, g.parse_reason) == ("device", "plain")
