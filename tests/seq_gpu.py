"""What the GPU tests of the packed-sequence codec share: a text taken to the device, the device entries run on it, the host
route and `fgfa`, each held against tests/seq_model.py byte for byte.  Imported by tests/test_gpu_seq.py and
tests/test_gpu_seq_geometry.py."""
import os
import subprocess

import numpy as np

import pollen_amd as pa
import seq_model as sm
from conftest import ROOT
from pollen_amd import _lib
from pollen_amd import device as pdev

FGFA = os.path.join(ROOT, "pollen_amd", "bin", "fgfa")


def as_array(text) -> np.ndarray:
    return text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), np.uint8)


def to_device(text):
    import torch
    return torch.from_numpy(as_array(text).copy()).to(torch.device("cuda:0"))


def want_of(text):
    """(the model's data bytes, its base count) of a text."""
    codes = sm.codes_of(as_array(text))
    return sm.pack_codes(codes).tobytes(), len(codes)


def check_device(text, what=""):
    """The device entries on a text: pack against the model, then unpack of the result against the kept letters."""
    data, n = want_of(text)
    packed, n_bases = pdev.seq_pack(to_device(text))
    assert n_bases == n, what
    assert packed.cpu().numpy().tobytes() == data, what
    letters = pdev.seq_unpack(packed, n_bases)
    assert letters.cpu().numpy().tobytes() == sm.unpack_codes(np.frombuffer(data, np.uint8), n).tobytes(), what
    return packed


def check_host(text, what=""):
    """The host routes: text to file image and back."""
    text = bytes(as_array(text))
    want = sm.export(text)
    image = pa.seq_export(text)
    assert image == want, what
    assert pa.seq_import(image) == sm.import_(want), what


def check_cli(text, tmp_path, what=""):
    text = bytes(as_array(text))
    src, out = tmp_path / "in.txt", tmp_path / "out.packed"
    src.write_bytes(text)
    r = subprocess.run([FGFA, "seq-export", str(src), str(out)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stdout == b"", (what, r.stderr)
    want = sm.export(text)
    assert out.read_bytes() == want, what
    r = subprocess.run([FGFA, "seq-import", str(out)], capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stdout == sm.import_(want) + b"\n", (what, r.stderr)


def export_error(text):
    """The code and message of the host route's refusal of a text."""
    try:
        pa.seq_export(bytes(as_array(text)))
    except pa.FlatGFAError as e:
        return e.code, _lib.last_error()
    raise AssertionError("not refused")


def pack_error(text_tensor):
    try:
        pdev.seq_pack(text_tensor)
    except pa.FlatGFAError as e:
        return e.code, _lib.last_error()
    raise AssertionError("not refused")


def bad_byte_message(byte, offset):
    return f"seq-export: byte 0x{byte:02x} at offset {offset} is not a nucleotide"
