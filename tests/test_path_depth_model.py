"""tests/path_depth_model.py and tests/path_depth_shapes.py pinned on the CPU: the model against the C oracle on the golden
graphs, on seeded synthetic ones and on every shape (a segment's length is a span of u32 offsets, so every shape fits the
oracle's pools); its rounding rule against hand-computed cases; its uint64 twin against the exact model; every shape's
declared carry sites from the model's reports, with the precondition that all totals stay below 2^64; and the kernels'
geometry constants the shapes mirror against the source text."""
import functools
import struct

import numpy as np
import pytest

import chop_shapes
import path_depth_model as pm
import path_depth_shapes as ps
from conftest import fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from oracle import synth

NAMES = [n for n, _ in ps.catalog()]


@functools.lru_cache(maxsize=None)
def shape(name: str) -> ps.Shape:
    return dict(ps.catalog())[name]()


def soa(pools: fo.Pools):
    return pools.steps, pools.paths["steps_start"], pools.paths["steps_end"], pools.seg_lens(), len(pools.segs)


def bits(x) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def check_against_oracle(pools: fo.Pools):
    ans = pm.exact(*soa(pools))
    want_len, want_mean = fo.path_depth(pools)
    assert ans.length == [int(x) for x in want_len]
    assert ans.mean.tobytes() == want_mean.tobytes()  # (bitwise: NaN included)
    assert (ans.depth == fo.seg_depth(pools)).all()
    tw = pm.twin(*soa(pools))
    assert tw.length.tolist() == ans.length and tw.weighted.tolist() == ans.weighted and tw.mean.tobytes() == ans.mean.tobytes()
    return ans


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_model_is_the_oracle_on_the_golden_graphs(gfa):
    with open(gfa, "rb") as f:
        check_against_oracle(fo.parse_gfa(f.read()))


def test_model_is_the_oracle_on_synthetic_graphs():
    for seed, (S, P, L, model) in enumerate([(500, 3, 4000, "pangenome"), (64, 1, 3000, "uniform"), (2000, 12, 700, "chromosome"),
                                             (300, 30, 90, "pangenome"), (50, 2, 5000, "repeats"), (7, 5, 1, "uniform")]):
        check_against_oracle(synth.pools(seed + 1, S, P, L, model))


@pytest.mark.parametrize("name", NAMES)
def test_model_is_the_oracle_on_every_shape(name):
    s = shape(name)
    want_len, want_mean = fo.path_depth(ps.pools_of(s))
    small = len(s.steps) <= ps.EXACT_MAX_STEPS
    tw = pm.twin(*s.graph())
    assert tw.length.tolist() == want_len.tolist() and tw.mean.tobytes() == want_mean.tobytes()
    if small:
        ans = pm.exact(*s.graph())
        assert ans.length == tw.length.tolist() and ans.weighted == tw.weighted.tolist() and ans.mean.tobytes() == tw.mean.tobytes()


def test_rounding_cases_by_hand():
    """u64 as f64 rounds to nearest, ties to even.  Above 2^53 the spacing is 2: 2^53 + 1 is a tie and goes to the even
    neighbour 2^53; 2^53 + 3 is a tie between 2^53 + 2 (odd mantissa) and 2^53 + 4 (even) and goes up.  2^64 - 1 is above the
    midpoint of 2^64 - 2048 and 2^64 and becomes 2^64."""
    one = 1
    assert bits(pm.mean_of(one, (1 << 53) + 1)) == bits(2.0 ** 53) == 0x4340000000000000
    assert bits(pm.mean_of(one, (1 << 53) + 3)) == bits(2.0 ** 53 + 4) == 0x4340000000000002
    assert bits(pm.mean_of(one, (1 << 64) - 1)) == bits(2.0 ** 64) == 0x43F0000000000000
    assert bits(pm.mean_of(one, (1 << 64) - 1024)) == bits(2.0 ** 64)  # (the midpoint: the tie goes to the even one, 2^64)
    assert bits(pm.mean_of(one, (1 << 64) - 1025)) == bits(2.0 ** 64 - 2048) == 0x43EFFFFFFFFFFFFF
    # both operands rounded, then one division: (2^53 + 1) / (2^53 + 3) is 2^53 / (2^53 + 4), below one by two ulps of 0.5
    assert bits(pm.mean_of((1 << 53) + 3, (1 << 53) + 1)) == bits(2.0 ** 53 / (2.0 ** 53 + 4)) == 0x3FEFFFFFFFFFFFFC
    assert pm.mean_of((1 << 64) - 1, (1 << 64) - 1) == 1.0 and pm.mean_of((1 << 53) + 1, 1 << 53) == 1.0
    nan = pm.mean_of(0, 0)
    assert np.isnan(nan)
    # the NaN of the oracle's own 0 / 0, bit for bit (an x86 division gives the negative quiet NaN, float("nan") the positive)
    p = chop_shapes.make_pools([0, 5], np.array([0], np.uint32), [(0, 1), (1, 1)], seq=False)
    _, want = fo.path_depth(p)
    assert want.tobytes() == np.array([nan, nan]).tobytes()
    assert bits(pm.mean_of(3, 0)) == 0 and pm.mean_of(1, 3) == 3.0


def test_twin_refuses_totals_beyond_64_bits():
    lens = np.array([ps.M32], np.uint32)
    steps = np.zeros(1 << 16, np.uint32)  # depth 65536: weighted = 65536^2 * (2^32 - 1) = 2^64 - 2^32 -- the last that fits
    tw = pm.twin(steps, [0], [1 << 16], lens, 1)
    assert int(tw.weighted[0]) == (1 << 64) - (1 << 32) == pm.exact(steps, [0], [1 << 16], lens, 1).weighted[0]
    steps = np.zeros((1 << 16) + 1, np.uint32)
    assert pm.exact(steps, [0], [len(steps)], lens, 1).weighted[0] >= 1 << 64
    with pytest.raises(AssertionError):
        pm.twin(steps, [0], [len(steps)], lens, 1)


def test_mirrored_constants_are_the_source_texts():
    c = ps.source_constants()
    for k, v in c.items():
        assert v == getattr(ps, k if k != "RUN_CAP_SCAN" else "RUN_CAP"), k
    assert ps.KPER == 4 and ps.WAVE_SEGS == 256 and ps.W == 4096
    assert pm.window_bits(ps.WB_LARGE_FROM) == ps.WB and pm.window_bits(ps.WB_LARGE_FROM + 1) == ps.WB_LARGE
    for n_cus in (256, 304, 64):
        full = ps.JOBS_PER_CU * n_cus
        assert pm.split_of(1, n_cus) == ps.MAX_SPLIT and pm.split_of(full, n_cus) == 1 and pm.split_of(full + 1, n_cus) == 1
        assert pm.split_of(full // 2, n_cus) == 2 and pm.split_of(10 * full, n_cus) == 1 and pm.split_of(full // 64, n_cus) == 64 and pm.split_of(full // 32, n_cus) == 32


@pytest.mark.parametrize("name", NAMES)
def test_shapes_carry_where_they_say(name):
    s = shape(name)
    assert s.sites and ps.verify(s) == len(s.sites)
    assert pm.window_bits(s.n_segs) == (ps.WB_LARGE if name == "large_windows" else ps.WB)
    assert int(s.seg_len.max()) >= 1 << 16 and len(s.steps) < 3_000_000


def test_what_the_shapes_cover():
    """The lists the GPU tests are built around, so that an edit of a shape that empties one fails here."""
    kinds = {}
    for n in NAMES:
        for site in shape(n).sites:
            kinds.setdefault(site[0], []).append((n,) + site[1:])
    assert [x[3] for x in kinds["prefix"]] == [1, ps.W - 1, 5 * ps.KPER, 3 * ps.WAVE_SEGS, 99]
    assert sorted(x[3] for x in kinds["run"]) == [1, 1, 1, 2, 700, 1023, ps.RUN_CAP]
    wt = shape("wave_totals")
    counts = [int(wt.end[p] - wt.begin[p]) for p in range(wt.P)]
    assert tuple(counts) == ps.RECORD_COUNTS == (2, 3, 4, 8, 16, 32, 64, 65, 200)
    mi = shape("many_items")
    assert mi.P > 64 * 16 and mi.P % 8 != 0 and (mi.P // 16) % 8 != 0
    assert {x[1] for x in kinds["gather_level"]} == {"thread", "wave", "block", "atomic"}
    gl = shape("gather_lengths")
    assert tuple(int(e - b) for b, e in zip(gl.begin, gl.end)) == ps.GATHER_STEPS
    assert [len(ids) for _, ids in gl.requests] == [13, 1, 13, 7, 4096, 4097, 3 * 4096 + 5]
    mx = shape("mixed")
    n = [int(e - b) for b, e in zip(mx.begin, mx.end)]
    assert max(n) > ps.SHORT_MAX and any(ps.TINY_MAX < x <= ps.SHORT_MAX for x in n) and any(0 < x <= ps.TINY_MAX for x in n)
    assert mx.n_segs <= ps.SHORT_MAX_SEGS
    assert len(kinds["near64"]) == 3 and len(kinds["nan"]) >= 4 and len(kinds["path_reduce"]) == 3 and len(kinds["split"]) == 2
