"""Every shape of tests/flatten_shapes.py builds, with its premise (asserted where it is built) holding on the model: the
GPU tests of the same shapes are then about the kernels, not about the shapes."""
import pytest

import flatten_model as fm
import flatten_shapes as fs


@pytest.mark.parametrize("name", list(fs.CATALOG))
def test_shape_builds(name):
    s = fs.CATALOG[name]()
    assert s.name == name
    p = s.pools
    assert len(fm.legend(p)) == len(p.segs) + 1
    n_lines = sum(int(q["steps_end"]) - int(q["steps_start"]) for q in p.paths)
    if s.chunk is not None:
        assert s.chunks == -(-n_lines // s.chunk) and s.chunks > 1
    else:
        assert n_lines <= fm.CHUNK_LINES


def test_bad_handle_is_bad():
    p = fs.bad_handle()
    assert int(p.steps[int(p.paths[-1]["steps_end"]) - 1]) >> 1 == len(p.segs)
