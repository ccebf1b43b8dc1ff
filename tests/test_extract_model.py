"""The sequential model of extract and position (tests/extract_model.py) against answers written out by hand from
flatgfa/src/ops/extract.rs, ops/position.rs and print.rs; and the host-only parts of the library's new surface."""
import pytest

import extract_model as em
import pollen_amd as pa
from extract_shapes import BY_NAME
from oracle import flatgfa_oracle as fo


def test_two_parents_by_hand():
    # level 1 pushes 2 then 3; level 2 pops 3 first: link 3 (3 -> 5) gives 5 the id 3, link 4 (3 -> 4) gives 4 the id 4
    sh = BY_NAME["two_parents_lifo"]
    got = em.text(em.extract_by_name(sh.pools(), 1, 2, iters=0))
    assert got == (b"H\tVN:Z:1.0\n"
                   b"S\t1\tAC\nS\t2\tCG\nS\t3\tGT\nS\t5\tAC\nS\t4\tTA\n"
                   b"P\tp:0-10\t1+,2+,4+,5+,3+\t*\n"
                   b"L\t1\t+\t2\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t2\t+\t4\t+\t0M\nL\t3\t+\t5\t+\t0M\nL\t3\t+\t4\t+\t0M\n")
    # one level only: 4 and 5 are not reached, the path falls into two runs, three links go
    got = em.text(em.extract_by_name(sh.pools(), 1, 1, iters=0))
    assert got == (b"H\tVN:Z:1.0\nS\t1\tAC\nS\t2\tCG\nS\t3\tGT\n"
                   b"P\tp:0-4\t1+,2+\t*\nP\tp:8-10\t3+\t*\n"
                   b"L\t1\t+\t2\t+\t0M\nL\t1\t+\t3\t+\t0M\n")


def test_c_zero_by_hand():
    got = em.text(em.extract_by_name(BY_NAME["c_zero"].pools(), 1, 0, iters=0))
    assert got == b"H\tVN:Z:1.0\nS\t1\tAC\nP\tp:0-2\t1+\t*\nP\tp:5-7\t1-\t*\nL\t1\t+\t1\t+\t0M\n"


def test_optional_data_alignment_and_merge_by_hand():
    gfa = (b"S\t1\tAC\tLN:i:2\nS\t2\tGGG\nS\t3\tT\tRC:i:7\tXX:Z:y\nS\t4\tAAAA\n"
           b"P\tx\t1+,2-,3+,4+\t2M,1M,0M\nL\t3\t+\t1\t+\t1M\nL\t2\t-\t3\t+\t0M\nL\t3\t+\t4\t+\t7M\nL\t1\t+\t1\t-\t3M2N\n")
    p = fo.parse_gfa(gfa)
    # {1}, and 3 through link 0 (to -> from); 2 lies in the gap 1 .. 3 re-entered at position 5 <= D; 4 stays outside
    want = (b"S\t1\tAC\tLN:i:2\nS\t3\tT\tRC:i:7\tXX:Z:y\nS\t2\tGGG\n"
            b"P\tx:0-6\t1+,2-,3+\t*\n"
            b"L\t3\t+\t1\t+\t1M\nL\t2\t-\t3\t+\t0M\nL\t1\t+\t1\t-\t3M2N\n")
    assert em.text(em.extract_by_name(p, 1, 1)) == want
    # D = 4: the re-entry at 5 is too far; 2 stays out and the path falls apart
    assert em.text(em.extract_by_name(p, 1, 1, max_dist=4)) == (b"S\t1\tAC\tLN:i:2\nS\t3\tT\tRC:i:7\tXX:Z:y\n"
                                                                 b"P\tx:0-2\t1+\t*\nP\tx:5-6\t3+\t*\n"
                                                                 b"L\t3\t+\t1\t+\t1M\nL\t1\t+\t1\t-\t3M2N\n")
    assert em.extract_by_name(p, 9, 1) is None  # "segment not found"


def test_model_print_matches_the_library_printer():
    for sh in BY_NAME.values():
        q = em.extract_by_name(sh.pools(), sh.n, sh.c, sh.d, sh.e)
        import chop_model as cm
        assert em.text(q) == cm.text(q), sh.name


def test_long_alignment_spans_print_like_short_ones():
    # past 4 096 ops _align formats every distinct op once: the same bytes as op by op
    import numpy as np
    rng = np.random.default_rng(0)
    p = fo.parse_gfa(b"S\t1\tAC\n")
    p.alignment = ((rng.integers(0, 1 << 24, 9000) << 8) | rng.integers(0, 4, 9000)).astype(np.uint32)
    for a, b in ((0, 9000), (17, 4114), (17, 4113)):
        assert em._align(p, a, b) == b"".join(b"%d%s" % (int(o) >> 8, "MNDI"[int(o) & 0xFF].encode()) for o in p.alignment[a:b])


def test_position_by_hand():
    p = fo.parse_gfa(b"S\t1\tAC\nS\t2\tGGG\nS\t7\tT\nP\tx\t1+,2-,7+\t*\nP\ty\t7-\t*\n")
    assert em.position(p, 0, 0) == (0, 0) and em.position(p, 0, 1) == (0, 1)
    assert em.position(p, 0, 2) == (3, 0) and em.position(p, 0, 4) == (3, 2)
    assert em.position(p, 0, 5) == (4, 0) and em.position(p, 0, 6) is None
    assert em.position_table(p, b"x,4,+") == b"#source.path.pos\ttarget.graph.pos\nx,4,+\t2,2,-\n"
    assert em.position_table(p, b"y,0,+") == b"#source.path.pos\ttarget.graph.pos\ny,0,+\t7,0,-\n"
    assert em.position_table(p, b"x,+05,+") == b"#source.path.pos\ttarget.graph.pos\nx,5,+\t7,0,+\n"
    assert em.position_table(p, b"x,6,+") == b""
    for bad, msg in [(b"x,1", "position must be path_name,offset,orientation"), (b"x,1,+,", "position must be path_name,offset,orientation"),
                     (b"x,-1,+", "offset must be a number"), (b"x,,+", "offset must be a number"), (b"x,1 ,+", "offset must be a number"),
                     (b"x,18446744073709551616,+", "offset must be a number"), (b"x,1,f", "orientation must be + or -"),
                     (b"z,1,+", "path not found"), (b"z,1,-", "path not found"), (b"x,1,-", "only + is implemented so far")]:
        with pytest.raises(em.PositionError, match=msg.replace("+", r"\+")):
            em.position_table(p, bad)


# ---- the library's host-only side: no device is touched ----
def test_library_find_seg():
    g = pa.parse_bytes(b"S\t5\tAC\nS\t7\tGGG\nS\t5\tTTTT\n")
    assert g.find_seg(5) == 0 and g.find_seg(7) == 1 and g.find_seg(6) is None and g.find_seg(2 ** 64 - 1) is None
    with pytest.raises(KeyError):
        g.extract(6, 1)


def test_library_position_argument_errors():
    gfa = b"S\t1\tAC\nS\t2\tGGG\nS\t7\tT\nP\tx\t1+,2-,7+\t*\nP\ty\t7-\t*\n"
    g, p = pa.parse_bytes(gfa), fo.parse_gfa(gfa)
    for bad in [b"x,1", b"x,1,+,", b"", b"x,-1,+", b"x,,+", b"x,1 ,+", b"x,18446744073709551616,+", b"x,1,f", b"z,1,+", b"z,1,-", b"x,1,-"]:
        with pytest.raises(em.PositionError) as want:
            em.position_table(p, bad)
        with pytest.raises(pa.FlatGFAError) as got:
            g.position_table(bad)
        assert got.value.code == -1 and str(want.value) in str(got.value), bad
    with pytest.raises(KeyError):
        g.position(b"z", 0)


def _random_gfa(seed, n_segs=40, n_paths=6, n_links=50):
    import numpy as np
    rng = np.random.default_rng(seed)
    lines = [b"H\tVN:Z:1.0"]
    for i in range(n_segs):
        lines.append(b"S\t%d\t%s" % (i + 1, bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 9))).astype(np.uint8))) + (b"\tLN:i:%d" % i if i % 5 == 0 else b""))
    o = lambda: b"+-"[int(rng.integers(0, 2)):][:1]  # noqa: E731
    for k in range(n_paths):
        n = int(rng.integers(1, 30))
        lines.append(b"P\tp%d\t" % k + b",".join(b"%d%s" % (int(rng.integers(1, n_segs + 1)), o()) for _ in range(n)) + b"\t*")
    for _ in range(n_links):
        a = int(rng.integers(1, n_segs + 1))
        b = a if rng.random() < 0.15 else int(rng.integers(1, n_segs + 1))
        lines.append(b"L\t%d\t%s\t%d\t%s\t%dM" % (a, o(), b, o(), int(rng.integers(0, 9))))
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("seed", range(8))
def test_fast_form_is_the_sequential_one(seed):
    import chop_model as cm
    p = fo.parse_gfa(_random_gfa(seed))
    for origin in range(0, len(p.segs), 7):
        for c in (0, 1, 2, 5):
            for d in (0, 6, 20, 300000):
                for e in (0, 1, 6):
                    assert cm.same_pools(em.extract(p, origin, c, d, e), em.extract_fast(p, origin, c, d, e)), (origin, c, d, e)
