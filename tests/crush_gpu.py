"""What the GPU tests of crush share: a sequence pool taken to the device, the device-level pair run on it, and its answer
held against tests/crush_model.py.  Imported by tests/test_gpu_crush.py and tests/test_gpu_crush_geometry.py."""
import numpy as np

import crush_model as cm
from oracle import flatgfa_oracle as fo
from pollen_amd import device as pdev


def device_graph_of(p: fo.Pools):
    lens = (p.segs["seq_end"] - p.segs["seq_start"]).astype(np.uint32)
    return pdev.DeviceGraph(p.steps, p.paths["steps_start"], p.paths["steps_end"], len(p.segs), lens)


def to_device(p: fo.Pools):
    import torch
    d = torch.device("cuda:0")
    seg_seq = torch.from_numpy(cm.seg_seq(p).view(np.int32)).to(d)
    seq = torch.from_numpy(np.ascontiguousarray(p.seq_data)).to(d)
    return device_graph_of(p), seg_seq, seq


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_device_pair(p: fo.Pools, want: fo.Pools, stream=None, what=""):
    """The device-level pair on p's sequence pool against the model's pools `want`; returns what pdev.crush returned."""
    dg, seg_seq, seq = to_device(p)
    new, seq_out, seg_seq_out = pdev.crush(dg, seg_seq, seq, stream=stream)
    if stream is not None:
        stream.synchronize()  # (that stream only)
    lens = (want.segs["seq_end"] - want.segs["seq_start"]).astype(np.uint32)
    assert np.array_equal(u32(new.seg_len), lens), what
    assert seq_out.cpu().numpy().tobytes() == want.seq_data.tobytes(), what
    spans = u32(seg_seq_out)
    assert np.array_equal(spans[0::2], want.segs["seq_start"]) and np.array_equal(spans[1::2], lens), what
    assert new.steps is dg.steps and new.path_begin is dg.path_begin and new.n_segs == dg.n_segs
    return new, seq_out, seg_seq_out
