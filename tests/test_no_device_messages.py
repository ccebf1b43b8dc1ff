"""What every GPU-only route says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and one sentence that names the
route ("no HIP device is visible; <route> has no CPU fallback").  The routes share the code that says it; the sentences
here are the ones each route spelt out for itself before they did.  Skipped where a device is visible."""
import pytest

import pollen_amd as pa
from pollen_amd import _lib

TEXT = b"S\t1\tACGT\nS\t2\tAC\nS\t3\tG\nP\tp\t1+,2+,3-\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t-\t0M\n"
GAF = b"r\t4\t0\t4\t+\t>1>2\t6\t0\t4\t4\t4\t60\n"

ROUTES = {
    "pangenotype": (lambda g: g.pangenotype_matrix([GAF]), "no HIP device is visible; the pangenotype matrix has no CPU fallback"),
    "gaf lookup": (lambda g: g.gaf_count(GAF), "no HIP device is visible; the GAF lookup has no CPU fallback"),
    "chop": (lambda g: g.chop(2, links=True), "no HIP device is visible; chop has no CPU fallback"),
    "extract": (lambda g: g.extract(1, 1), "no HIP device is visible; extract has no CPU fallback"),
    "position": (lambda g: g.position(b"p", 1), "no HIP device is visible; position has no CPU fallback"),
    "validate": (lambda g: g.validate(), "no HIP device is visible; validate has no CPU fallback"),
    "degree": (lambda g: g.degree(), "no HIP device is visible; degree has no CPU fallback"),
    # (no route with a scope of its own: the depth queries say it through the same helper)
    "depth": (lambda g: g.seg_depth(), "no HIP device is visible; the depth queries have no CPU fallback"),
}


@pytest.mark.parametrize("what", list(ROUTES))
def test_no_device_message(what):
    call, message = ROUTES[what]
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    assert g.segment_count == 3
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            call(g)
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == message
    finally:
        g.close()
