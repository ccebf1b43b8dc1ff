"""The build of the sorted record image on its own (pollen_amd/csrc/depth_sorted.hip: sorted_image_count, sorted_image_emit,
sorted_image_finalise and the host between them), run by the stand-alone program tests/device_check/sorted_image_check.hip
(built with the library: `make -C pollen_amd/csrc sorted_image_check`) over the cases of tests/sorted_image_cases.py: hand-made
plans of a few hundred records that reach what whole plans do not -- one CU's grid, items of more than 256 entries, more than
8192 windows, every refusal -- and what the finaliser leaves that no answer depends on.  The program runs once for the whole
module, every case in one process, refusals between builds; each test then holds one case's dump to the model
(tests/test_sorted_image_cases.py ties that model to brute force without a GPU).  Run with -m gpu."""
import os
import subprocess

import pytest

import sorted_image_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
EXE = os.path.join(ROOT, "pollen_amd", "build", "sorted_image_check")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    subprocess.run(["make", "-C", CSRC, "sorted_image_check"], check=True, capture_output=True, timeout=600)
    d = tmp_path_factory.mktemp("sorted_image_check")
    lines, paths = [], {}
    for k, c in enumerate(sc.CASES):
        src, dst = d / ("%d.in" % k), d / ("%d.out" % k)
        src.write_bytes(c.make_input())
        lines.append("%s %s\n" % (src, dst))
        paths[c.id] = dst
    manifest = d / "manifest.txt"
    manifest.write_text("".join(lines))
    r = subprocess.run([EXE, str(manifest)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == "sorted_image_check: %d cases" % len(sc.CASES)
    for k in range(len(sc.CASES)):
        (d / ("%d.in" % k)).unlink()
    return paths


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_case(outputs, case):
    case.check(outputs[case.id].read_bytes())
