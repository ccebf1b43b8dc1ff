"""tools/seq_cpu.cpp, the single-thread C++ restatement that tools/seq_bench.py times, held against tests/seq_model.py: it
writes the model's file image and the model's bases, and refuses what the model refuses.  No GPU."""
import os
import shutil
import subprocess

import pytest

import seq_model as sm
import seq_shapes as ss
from conftest import ROOT


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("seq_cpu") / "seq_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tools", "seq_cpu.cpp"), "-o", out], check=True)
    return out


def run(tool, d, mode, data):
    src, out = d / "in.bin", d / "out.bin"
    src.write_bytes(data)
    if out.exists():
        out.unlink()
    return subprocess.run([tool, mode, str(src), str(out)], capture_output=True, timeout=120), out


def test_round_trips(tool, tmp_path):
    texts = [b"ACTGG\n", b"", b" \n"] + list(ss.CHUNK_TEXTS.values()) + [bytes(ss.sprinkled(n, 0.2, n)) for n in (1, 2, 63, 64, 65, 5000)]
    for text in texts:
        r, out = run(tool, tmp_path, "export", text)
        assert r.returncode == 0, r.stderr
        image = out.read_bytes()
        assert image == sm.export(text) and int(r.stdout.split()[0]) == sm.packed_info(image)[0]
        r, out = run(tool, tmp_path, "import", image)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == sm.import_(image) and int(r.stdout.split()[0]) == len(sm.import_(image))


@pytest.mark.parametrize("bad", [b"a", b"N", b"\0", b"\xff", b"\x0b"])
def test_export_refuses(tool, tmp_path, bad):
    r, out = run(tool, tmp_path, "export", b"ACGT \n" + bad + b"AC" + bad)
    assert r.returncode == 3 and f"byte 0x{bad[0]:02x} at offset 6".encode() in r.stderr and not out.exists()


def test_import_refuses_and_accepts(tool, tmp_path):
    for name, file in ss.REFUSED.items():
        r, out = run(tool, tmp_path, "import", file)
        assert r.returncode == 3 and not out.exists(), name
    for name, (file, want) in ss.ACCEPTED.items():
        r, out = run(tool, tmp_path, "import", file)
        assert r.returncode == 0 and out.read_bytes() == want, name
    r, out = run(tool, tmp_path, "import", ss.hdr(length=3, capacity=3, hne=1) + bytes([0x10, 0x42, 0x34]))
    assert r.returncode == 3 and b"nibble 4 at base 3" in r.stderr and not out.exists()
