"""slow_odgi's validate (slow_odgi/validate.py:5-25) and degree (slow_odgi/degree.py:5-18), both over the adjacency lists of
mygfa/preprocess.py:23-43, restated over the pools of oracle.flatgfa_oracle.Pools in numpy.  tests/test_topology_model.py pins
this to the reference's own output (tests/golden/topology/); the GPU tests compare the library with it byte for byte.

Handles are the pools' own: segment id << 1 | backward, flip(h) = h ^ 1."""
import numpy as np

from oracle import flatgfa_oracle as fo

REC_DT = np.dtype([("path", "<u4"), ("step", "<u4"), ("src", "<u4"), ("dst", "<u4")])


def _key(a, b):
    return (np.asarray(a, np.uint64) << np.uint64(32)) | np.asarray(b, np.uint64)


def link_keys(p: fo.Pools) -> np.ndarray:
    """Every link in both of its equivalent forms, sorted: (from, to) and (flip(to), flip(from))."""
    f, t = p.links["from_"].astype(np.uint64), p.links["to"].astype(np.uint64)
    return np.unique(np.concatenate([_key(f, t), _key(t ^ np.uint64(1), f ^ np.uint64(1))]))


def validate(p: fo.Pools) -> np.ndarray:
    """One record per consecutive pair of steps of a path that is not in outs (validate.py:13-19), paths in pool order."""
    keys = link_keys(p)
    out = []
    for i, path in enumerate(p.paths):
        st = p.steps[int(path["steps_start"]):int(path["steps_end"])]
        if len(st) < 2:  # validate.py:11-12
            continue
        k = _key(st[:-1], st[1:])
        at = np.searchsorted(keys, k)
        found = np.zeros(len(k), bool)
        ok = at < len(keys)
        found[ok] = keys[at[ok]] == k[ok]
        miss = np.flatnonzero(~found)
        r = np.zeros(len(miss), REC_DT)
        r["path"], r["step"], r["src"], r["dst"] = i, miss, st[miss], st[miss + 1]
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, REC_DT)


def _handle(p: fo.Pools, h: int) -> bytes:
    return b"%d%s" % (int(p.segs[h >> 1]["name"]), b"-" if h & 1 else b"+")


def records_text(p: fo.Pools, recs: np.ndarray) -> bytes:
    """validate.py:20-24"""
    return b"".join(b"[odgi::validate] error: the path %s does not respect the graph topology: the link %s,%s is missing.\n"
                    % (p.path_name(int(r["path"])), _handle(p, int(r["src"])), _handle(p, int(r["dst"]))) for r in recs)


def validate_text(p: fo.Pools) -> bytes:
    return records_text(p, validate(p))


def degree(p: fo.Pools) -> np.ndarray:
    """degree.py:11-16: the lengths of the four lists of a segment -- every link counts once at its `from` and once at its `to`."""
    S = len(p.segs)
    return (np.bincount(p.links["from_"] >> 1, minlength=S) + np.bincount(p.links["to"] >> 1, minlength=S)).astype(np.uint64)[:max(S, 0)]


def degree_text(p: fo.Pools) -> bytes:
    """degree.py:7, 17"""
    d = degree(p)
    return b"#node.id\tnode.degree\n" + b"".join(b"%d\t%d\n" % (int(s["name"]), int(d[i])) for i, s in enumerate(p.segs))
