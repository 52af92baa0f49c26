"""The expected value of the leave-one-out search (include/nsid.h nsid_flat_l2_topk_excl): row i's result is the plain search over the
database with rows [lo, hi) deleted, the ids mapped back. These helpers do the deletion and the mapping; the search itself is always
the plain entry's (tests/test_search_excl_gpu.py) or a brute force (tests/test_search_excl_cpu.py)."""
import numpy as np


def effective_range(lo, hi, nx):
    """the database rows a pair of ints excludes: [max(lo, 0), min(hi, nx)), or (0, 0) when that is empty"""
    lo, hi = max(int(lo), 0), min(int(hi), int(nx))
    return (lo, hi) if lo < hi else (0, 0)


def kept_rows(lo, hi, nx):
    """ids of the database rows that remain, ascending"""
    lo, hi = effective_range(lo, hi, nx)
    return np.concatenate([np.arange(0, lo), np.arange(hi, nx)]).astype(np.int64)


def map_back(I, lo, hi):
    """ids of a search over the compacted database -> ids of the full one: ids >= lo move up by hi - lo, -1 (no row) stays"""
    I = np.asarray(I, dtype=np.int64)
    return np.where(I >= lo, I + (hi - lo), I)


def groups(lo, hi, nx):
    """the query rows of a call grouped by their effective range: [((lo, hi), row ids)], for one plain search per group"""
    eff = [effective_range(a, b, nx) for a, b in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())]
    out = {}
    for i, r in enumerate(eff):
        out.setdefault(r, []).append(i)
    return [(r, np.asarray(rows, dtype=np.int64)) for r, rows in out.items()]


def brute_force(q, x, k, lo, hi):
    """fp64 brute force with the excluded rows deleted from the candidates of each query row: (D, I), ties to the smaller id,
    I = -1 / D = inf past the rows that remain"""
    q, x = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    nq, nx = q.shape[0], x.shape[0]
    D = np.full((nq, k), np.inf)
    I = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        cand = [j for j in range(nx) if not (lo[i] <= j < hi[i])]
        dist = [float(((q[i] - x[j]) ** 2).sum()) for j in cand]
        order = sorted(range(len(cand)), key=lambda t: (dist[t], cand[t]))[:k]
        for s, t in enumerate(order):
            D[i, s], I[i, s] = dist[t], cand[t]
    return D, I
