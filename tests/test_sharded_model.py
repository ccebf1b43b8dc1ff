"""tests/sharded_model.py and tests/sharded_shapes.py pinned on the CPU: the model's reduced vectors and path depths against
the oracle on the golden graphs and on seeded synthetic ones for many shard counts, its cut rule against the library's
host-only flatgfa_shard_cuts (lengths with totals beyond 2^56 among them), every closed form of the shapes against the
model, and the numbers of cut paths and packed words the GPU tests are built around."""
import numpy as np
import pytest

import pollen_amd as pa
import sharded_model as sm
import sharded_shapes as ss
from conftest import fixture_id, golden_gfas
from oracle import flatgfa_oracle as fo
from oracle import synth

SHARDS = [1, 2, 3, 5, 8, 13, 20, 64]


def check_against_oracle(pools, n_shards, flags=0):
    g = sm.graph_of(pools)
    lay = sm.layout(g, n_shards, flags)
    d, u, packed = sm.exchange(g, lay)
    want_d, want_u = fo.seg_depth_with_uniq(pools)
    assert (d == want_d).all() and (u == want_u).all()
    ln, mean = sm.path_depth(g, lay, d)
    want_ln, want_mean = fo.path_depth(pools)
    assert (ln == want_ln).all() and mean.tobytes() == want_mean.tobytes()  # (bitwise: NaN included)
    assert packed.shape == (lay.W, g.S)
    return lay


@pytest.mark.parametrize("gfa", golden_gfas(), ids=fixture_id)
def test_model_is_the_oracle_on_the_golden_graphs(gfa):
    with open(gfa, "rb") as f:
        pools = fo.parse_gfa(f.read())
    for n in SHARDS:
        for flags in (0, sm.WHOLE_PATHS):
            lay = check_against_oracle(pools, n, flags)
            assert lay.ordered and (not flags or lay.K == 0)


@pytest.mark.parametrize("n_shards", SHARDS)
def test_model_is_the_oracle_on_synthetic_graphs(n_shards):
    cut = 0
    for seed, (S, P, L, model) in enumerate([(500, 3, 4000, "pangenome"), (64, 1, 3000, "uniform"), (2000, 12, 700, "chromosome"),
                                             (300, 30, 90, "pangenome"), (50, 2, 5000, "repeats"), (7, 5, 1, "uniform")]):
        lay = check_against_oracle(synth.pools(seed + 1, S, P, L, model), n_shards)
        cut += lay.K
    assert (cut > 0) == (n_shards > 1)


def test_model_is_the_oracle_on_paths_out_of_pool_order():
    for kind in ss.OUT_OF_ORDER:
        for n in SHARDS:
            s = ss.out_of_order(kind, n)
            lay = check_against_oracle(ss.pools(s.graph), n)
            assert lay.ordered == s.ordered
            if not s.ordered:  # never cut, and a shard's slice covers its paths wherever they lie
                assert lay.K == 0 and lay.W == 0
                for sh in lay.shards:
                    assert all((x, y) == (s.graph.begin[p], s.graph.end[p]) for p, x, y in sh.pieces)
                    if sh.pieces:
                        assert sh.step_begin == min(x for _, x, _ in sh.pieces) and sh.step_end == max(y for _, _, y in sh.pieces)
    # the ordered graph with empty paths where the cuts fall is cut at them, not inside a path
    s = ss.out_of_order("ordered-empties", 4)
    lay = sm.layout(s.graph, s.n_shards)
    assert lay.cuts == (0, 500, 1000, 1500, 2000) and lay.K == 0 and [len(x.pieces) for x in lay.shards] == [1, 1, 1, 1]
    assert [x.first_path for x in lay.shards] == [1, 4, 6, 8]
    assert sm.layout(s.graph, 3).K == 2


def test_slices_of_a_reversed_pool():
    s = ss.out_of_order("reversed", 3)
    lay = sm.layout(s.graph, 3)
    assert not lay.ordered
    # shard 0 holds the first paths, which lie at the END of the pool
    assert lay.shards[0].first_path == 0 and lay.shards[0].step_end == int(s.graph.end[0])
    assert lay.shards[-1].step_begin == int(s.graph.begin[6]) == 3
    assert sum(len(x.pieces) for x in lay.shards) == 7


# ---- the cut rule ----
def lib_cuts(lens, n, flags=0):
    return [int(x) for x in pa.shard_cuts(np.array(lens, np.uint64), n, flags)]


def test_cuts_are_the_librarys_on_the_lengths_test_sharded_draws():
    rng = np.random.default_rng(11)  # (tests/test_sharded.py: test_c_route_cuts_are_shard_paths_cuts)
    for world in (1, 2, 3, 4, 8):
        for P in (0, 1, 2, 7, 8, 100, 1000):
            for hi_len in (1, 5000, 1_000_000):
                lens = [int(x) for x in rng.integers(0, hi_len + 1, size=P)]
                assert sm.cuts(lens, world) == lib_cuts(lens, world), (world, P, hi_len)
                assert sm.cuts(lens, world, True) == lib_cuts(lens, world, pa.SHARD_WHOLE_PATHS), (world, P, hi_len)


@pytest.mark.parametrize("case", [c for c in ss.cut_lengths() if not c[0].startswith("huge")], ids=lambda c: c[0])
def test_cuts_of_planted_lengths(case):
    _, lens, n = case
    assert sm.cuts(lens, n) == lib_cuts(lens, n)
    assert sm.cuts(lens, n, True) == lib_cuts(lens, n, pa.SHARD_WHOLE_PATHS)


@pytest.mark.parametrize("case", [c for c in ss.cut_lengths() if c[0].startswith("huge")], ids=lambda c: c[0])
def test_cuts_of_huge_lengths(case):
    """Totals from 2^56 on: the distance of the nearest boundary, times 8 n_shards, passes 2^64.  Compared in 64 bits the
    product wrapped to a small number and a boundary a third of the total away counted as near."""
    name, lens, n = case
    T = sum(lens)
    assert T < 1 << 64
    want = sm.cuts(lens, n)
    print(name, "model", want, "library", lib_cuts(lens, n))
    assert lib_cuts(lens, n) == want
    assert sm.cuts(lens, n, True) == lib_cuts(lens, n, pa.SHARD_WHOLE_PATHS)
    if name == "huge-one-path-3":
        assert want == [0, T // 3, 2 * T // 3, T]
    if len(lens) == 1:  # one path: no boundary but its ends, every shard an even share
        assert want[1:-1] == [T * r // n for r in range(1, n)]


def test_cuts_refuse_a_total_beyond_64_bits():
    """The cut points are u64: path lengths that add up to 2^64 or more have none, and are refused."""
    for lens in ([1 << 63, 1 << 63], [(1 << 64) - 1, 1], [1 << 62] * 5):
        with pytest.raises(pa.FlatGFAError) as ei:
            pa.shard_cuts(np.array(lens, np.uint64), 3)
        assert ei.value.code == ss.ERR_TOO_LARGE
    assert lib_cuts([(1 << 64) - 1], 2) == [0, (1 << 63) - 1, (1 << 64) - 1] == sm.cuts([(1 << 64) - 1], 2)
    assert lib_cuts([(1 << 63) - 1, 1 << 63], 4) == sm.cuts([(1 << 63) - 1, 1 << 63], 4)


# ---- the shapes ----
def closed_form(s: ss.Shape):
    lay = sm.layout(s.graph, s.n_shards, s.flags)
    d, u, packed = sm.exchange(s.graph, lay)
    if s.depth is not None:
        assert (d == s.depth).all() and (u == s.uniq).all(), s.name
    if s.K is not None:
        assert (lay.K, lay.W) == (s.K, s.W), (s.name, lay.K, lay.W)
    return lay, packed


@pytest.mark.parametrize("P,n_shards,K,W", ss.RINGS_MULTIWORD)
def test_rings_fill_more_than_one_word(P, n_shards, K, W):
    """The numbers of cut paths and of packed words the multi-word GPU tests rely on: a change of the cut rule that turned
    them back into one-word tests fails here."""
    s = ss.ring_multiword(P, n_shards, K, W)
    lay, packed = closed_form(s)
    assert (lay.K, lay.W) == (K, W) and W > 1
    assert lay.bits == {13: 4, 20: 5, 64: 7}[n_shards] and lay.per_word == {13: 8, 20: 6, 64: 4}[n_shards]
    assert lay.collective_bytes(True) == 4 * s.graph.S * (2 + W) and lay.collective_bytes(False) == 4 * s.graph.S
    S = s.graph.S
    for sh in lay.shards:
        assert all(y - x >= S for _, x, y in sh.pieces)  # every piece goes round the ring
    m = sm.fields(lay, packed)
    assert (m == 2).all()  # every cut path is in two pieces, both on every segment: the last field of a word and the first of the next among them
    want = sum(2 << ((k % lay.per_word) * lay.bits) for k in range(min(K, lay.per_word)))
    assert (packed[0] == want).all() and (packed[W - 1] != 0).all()
    assert want >> ((lay.per_word - 1) * lay.bits) == 2  # (shift 28 at 4 bits, 25 at 5, 21 at 7)
    assert (lay.per_word - 1) * lay.bits == {13: 28, 20: 25, 64: 21}[n_shards]
    d, u = fo.seg_depth_with_uniq(ss.pools(s.graph))
    assert (d == s.depth).all() and (u == s.uniq).all()


@pytest.mark.parametrize("n_shards", ss.RING_SINGLE)
def test_one_path_in_n_shards_pieces_counts_to_n_shards(n_shards):
    s = ss.ring_single(n_shards)
    lay, packed = closed_form(s)
    assert lay.K == 1 and lay.W == 1 and [len(x.pieces) for x in lay.shards] == [1] * n_shards
    assert (packed[0] == n_shards).all()  # the count is n_shards itself ...
    if n_shards & (n_shards - 1) == 0:
        assert n_shards >> (lay.bits - 1) == 1  # ... which needs the top bit of the field at a power of two
    assert 2 ** (lay.bits - 1) <= n_shards < 2 ** lay.bits


@pytest.mark.parametrize("P,n_shards,K,W", ss.RINGS_MULTIWORD + [(1, 8, 1, 1), (3, 16, 3, 1)])
def test_spokes_count_from_nothing_to_every_piece(P, n_shards, K, W):
    s = ss.spokes(P, n_shards, K, W)
    lay, packed = closed_form(s)
    check_against_oracle(ss.pools(s.graph), n_shards)
    m = sm.fields(lay, packed)
    pieces = {}
    for sh in lay.shards:
        for p, _, _ in sh.pieces:
            pieces[p] = pieces.get(p, 0) + 1
    for k, p in enumerate(lay.split_paths):
        hub = 2 * 960 + 3 * p
        assert m[k, hub] == pieces[p] == m[k].max() >= 2 and m[k].min() == 0
        assert 1 in m[k] and (pieces[p] == 2 or len(np.unique(m[k])) >= 4)  # nothing, one piece, some pieces, every piece
    if P == 1:
        assert pieces == {0: n_shards}


@pytest.mark.parametrize("S", [600, 2 * 256 + 300, 10_000])
def test_wide_in_small(S):
    s = ss.wide(S)
    lay, packed = closed_form(s)
    assert lay.split_paths == (0, 1, 2) and lay.cuts == (0, 3 * S // 2, 3 * S, 9 * S // 2, 6 * S)
    m = sm.fields(lay, packed)
    # path 0 is cut after a lap and a half, path 1 between its laps, path 2 half a lap in: the last segments -- those
    # beyond one grid trip at full size -- are touched by both pieces of paths 0 and 1 and by one piece of path 2
    assert (m[1] == 2).all() and (m[0, S // 2:] == 2).all() and (m[0, :S // 2] == 1).all()
    assert (m[2, :S // 2] == 2).all() and (m[2, S // 2:] == 1).all() and S - 300 >= S // 2
    d, u = fo.seg_depth_with_uniq(ss.pools(s.graph))
    assert (d == s.depth).all() and (u == s.uniq).all()


def test_wide_passes_one_grid_trip():
    assert ss.WIDE_SEGS == 2048 * 256 + 300 and ss.WIDE_SEGS % 2 == 0
    # (the full size, cuts only: the model runs it whole in the GPU suite)
    lens = [2 * ss.WIDE_SEGS] * 3
    assert sm.cuts(lens, 4) == [0, 3 * ss.WIDE_SEGS // 2, 3 * ss.WIDE_SEGS, 9 * ss.WIDE_SEGS // 2, 6 * ss.WIDE_SEGS]
