"""What the GPU tests of flip share: a graph image and its links taken to the device, the device-level pair run on them, and
its answer held against tests/flip_model.py.  Imported by tests/test_gpu_flip.py and tests/test_gpu_flip_geometry.py."""
import numpy as np

import flip_model as fm
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def to_device(p: fo.Pools):
    """(DeviceGraph, links, alignment) of these pools on device 0."""
    import torch
    d = torch.device("cuda:0")
    lens = (p.segs["seq_end"] - p.segs["seq_start"]).astype(np.uint32)
    dg = pdev.DeviceGraph(p.steps, p.paths["steps_start"], p.paths["steps_end"], len(p.segs), lens)
    links = torch.from_numpy(np.ascontiguousarray(p.links).view(np.uint32).view(np.int32).reshape(-1).copy()).to(d)
    align = torch.from_numpy(np.ascontiguousarray(p.alignment, dtype=np.uint32).view(np.int32).copy()).to(d)
    return dg, links, align


def check_device_pair(p: fo.Pools, want: fo.Pools, stream=None, what=""):
    """The device-level pair on p's image against the model's pools `want`; returns what pdev.flip returned."""
    dg, links, align = to_device(p)
    new, links_out, turned = pdev.flip(dg, links, stream=stream, alignment=align)
    if stream is not None:
        stream.synchronize()  # (that stream only)
    assert np.array_equal(u32(new.steps), want.steps), what
    assert np.array_equal(u32(turned).astype(bool), fm.turned(p)), what
    assert u32(links_out).tobytes() == want.links.tobytes(), what
    assert np.array_equal(new.h_path_begin, want.paths["steps_start"]) and np.array_equal(new.h_path_end, want.paths["steps_end"]), what
    assert np.array_equal(u32(new.path_begin), want.paths["steps_start"]) and np.array_equal(u32(new.path_end), want.paths["steps_end"]), what
    assert new.seg_len is dg.seg_len and new.n_segs == dg.n_segs and new.n_paths == dg.n_paths
    return new, links_out, turned


def check_handle(p: fo.Pools, want: fo.Pools, what=""):
    """flatgfa_flip and flatgfa_flip_count on a handle over p against the model's pools."""
    with fm.handle_of(p) as g:
        q = g.flip()
        try:
            fm.assert_same_pools(fm.pools_of(q), want, what)
            assert g.flip_count() == (int(fm.turned(p).sum()), len(want.links)), what
        finally:
            q.close()
