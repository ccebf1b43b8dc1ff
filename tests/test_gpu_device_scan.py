"""pollen_amd/csrc/device_scan.hpp on its own: the wave and workgroup scans, the three-launch tiled scan at every template
point a feature uses or is about to, last_start_at_or_before and k_check_links, run by the stand-alone program
tests/device_check/scan_check.hip (built with the library: `make -C pollen_amd/csrc scan_check`) over the cases of
tests/device_scan_cases.py.  The program runs once for the whole module, every case in one process; each test then compares
one case's output, guard elements included, with the reference.  Run with -m gpu."""
import os
import subprocess

import pytest

import device_scan_cases as dc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "pollen_amd", "csrc")
EXE = os.path.join(ROOT, "pollen_amd", "build", "scan_check")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    subprocess.run(["make", "-C", CSRC, "scan_check"], check=True, capture_output=True, timeout=600)
    d = tmp_path_factory.mktemp("scan_check")
    lines, paths = [], {}
    for k, c in enumerate(dc.CASES):
        src, dst = d / ("%d.in" % k), d / ("%d.out" % k)
        src.write_bytes(c.make_input())
        lines.append("%s %s %d %s %s\n" % (c.kind, c.point, c.n, src, dst))
        paths[c.id] = dst
    manifest = d / "manifest.txt"
    manifest.write_text("".join(lines))
    r = subprocess.run([EXE, str(manifest)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == "scan_check: %d cases" % len(dc.CASES)
    for k in range(len(dc.CASES)):
        (d / ("%d.in" % k)).unlink()
    return paths


def test_every_case_has_its_own_id():
    assert len({c.id for c in dc.CASES}) == len(dc.CASES)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.id)
def test_case(outputs, case):
    case.check(outputs[case.id].read_bytes())
