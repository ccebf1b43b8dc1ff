"""What interval depth over many paths says on a machine without a HIP device: FLATGFA_ERR_NO_DEVICE and the sentence every
GPU-only route says ("no HIP device is visible; <route> has no CPU fallback", tests/test_no_device_messages.py).  Skipped
where a device is visible."""
import pytest

import pollen_amd as pa
from pollen_amd import _lib

TEXT = b"S\t1\tACGT\nS\t2\tAC\nS\t3\tG\nP\tp\t1+,2+,3-\t*\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t-\t0M\n"

ROUTES = {
    "intervals": (lambda g: g.intervals_depth([0], [0], [4]), "no HIP device is visible; interval depth has no CPU fallback"),
    "window table": (lambda g: g.window_depth_paths_table(4), "no HIP device is visible; window depth has no CPU fallback"),
    "bed table": (lambda g: g.bed_depth_paths_table(b"p\t0\t4\n"), "no HIP device is visible; interval depth has no CPU fallback"),
}


@pytest.mark.parametrize("what", list(ROUTES))
def test_no_device_message(what):
    call, message = ROUTES[what]
    if pa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = pa.parse_bytes(TEXT)
    try:
        with pytest.raises(pa.FlatGFAError) as e:
            call(g)
        assert e.value.code == -3  # FLATGFA_ERR_NO_DEVICE
        assert _lib.last_error() == message
        # what needs no device is answered without one
        assert len(g.intervals_depth([], [], [])) == 0
        with pytest.raises(pa.FlatGFAError) as e:
            g.intervals_depth([5], [0], [4])
        assert e.value.code == -2
    finally:
        g.close()
