"""The oracle of the normalised candidate search (include/nsid.h, "normalised candidate search"): the rule in numpy on top of
score_norm_oracle (the exact fp32 chain, the ordered fp64 sums, the five roundings of the cell), and the generator of the retrieval
hub case. The diagonal vote is diag_vote_oracle's and the alignment locate_oracle's: nothing of them is restated here."""
import functools

import numpy as np

from locate_oracle import smooth_rows
from score_norm_oracle import chain_dot, cohort_stats, norm_cells


# ---------------------------------------------------------------------------------------------------- the rule
def norm_topk(z, k, lo=None, hi=None):
    """z (nq, nx) fp32 scores -> (Z (nq, k) fp32, I (nq, k) int64): per row the k largest z, a stable sort by (-z, id) (so +0 and -0
    tie and go by id), NaN dropped, rows lo[i] <= j < hi[i] dropped, the tail I = -1, Z = -inf"""
    z = np.asarray(z, dtype=np.float32)
    nq, nx = z.shape
    Z = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(nx)
    for i in range(nq):
        keep = ~np.isnan(z[i])
        if lo is not None:
            keep &= ~((ids >= int(lo[i])) & (ids < int(hi[i])))
        cand = ids[keep]
        order = cand[np.argsort(-z[i][cand], kind="stable")][:k]
        Z[i, :order.size] = z[i][order]
        I[i, :order.size] = order
    return Z, I


def scores(q, x, q_stats, x_stats):
    """z (nq, nx): pair_sim_norm's cell of every (query row, database row), in the oracle's own arithmetic"""
    return norm_cells(chain_dot(q, x), *q_stats, *x_stats)


def flat_norm_topk(q, x, q_stats, x_stats, k, lo=None, hi=None):
    return norm_topk(scores(q, x, q_stats, x_stats), k, lo, hi)


def raw_topk(S, x, k):
    """the L2 search's lists from the dots S (nq, nx): key ||x_j||^2 - 2 s in fp32, ties to the smaller id"""
    xn = (np.asarray(x, dtype=np.float64) ** 2).sum(1).astype(np.float32)
    key = xn[None, :] - (S + S)
    return np.argsort(key, axis=1, kind="stable")[:, :k].astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the retrieval hub case
HUB_D = 128
HUB_DUMMY, HUB_DUMMY_SHARE = 1024, 0.15
HUB_SONGS, HUB_SONG_ROWS = 12, 64
HUB_GENERIC_SONGS, HUB_GENERIC_ROWS = range(4, 12), (16, 48)        # songs 4-11, rows 16-47
HUB_QUERY_ROWS, HUB_PLANT = 48, (0, 32, 2, 10)                      # query rows 0-31 = song 2 rows 10-41
HUB_PLANT_NOISE, HUB_PLANT_U = 0.5, 1.5
HUB_COHORT = 512
HUB_SEEDS = range(6)
HUB_K = 20
HUB_THETA, HUB_MIN_SCORE = 2.5, 10.0


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def hub_case(seed):
    """(dummy (1024, d), songs [12 x (64, d)], query (48, d)) fp32. One PCG64 generator, drawn in this order: u; the dummy rows, the
    positions of their generic rows (rng.choice), those generic rows; per song its rows, then (songs 4-11) its generic rows; the
    query's rows, then per planted row t its noise g. A generic row is unit(2 u + g / sqrt(d)), g standard normal."""
    d = HUB_D
    rng = np.random.Generator(np.random.PCG64(seed))
    u = _unit(rng.standard_normal(d)).astype(np.float64)

    def generic(n):
        return _unit(2.0 * u[None, :] + rng.standard_normal((n, d)) / np.sqrt(d))

    dummy = smooth_rows(rng, HUB_DUMMY, d)
    which = rng.choice(HUB_DUMMY, size=int(round(HUB_DUMMY_SHARE * HUB_DUMMY)), replace=False)
    dummy[which] = generic(which.size)
    songs = []
    for s in range(HUB_SONGS):
        rows = smooth_rows(rng, HUB_SONG_ROWS, d)
        if s in HUB_GENERIC_SONGS:
            rows[HUB_GENERIC_ROWS[0]:HUB_GENERIC_ROWS[1]] = generic(HUB_GENERIC_ROWS[1] - HUB_GENERIC_ROWS[0])
        songs.append(rows)
    query = smooth_rows(rng, HUB_QUERY_ROWS, d)
    a, n, song, b = HUB_PLANT
    for t in range(n):
        g = rng.standard_normal(d)
        query[a + t] = _unit(songs[song][b + t].astype(np.float64) + HUB_PLANT_NOISE * g / np.sqrt(d) + HUB_PLANT_U * u)
    return dummy, songs, query


def default_cohort(dummy, size=HUB_COHORT):
    """SampleIndex.set_cohort(size=...) without rows: the dummy rows at positions floor(m n_dummy / M)"""
    M = min(size, dummy.shape[0])
    return dummy[(np.arange(M, dtype=np.int64) * dummy.shape[0]) // M]


@functools.lru_cache(maxsize=None)
def hub(seed):
    """everything the tests need of one seed, computed once: the rows, the index (dummy ++ songs) with its song codes, the exact dots
    S (query x index), the statistics of the query and of every index row against the default cohort, and the normalised scores z"""
    dummy, songs, query = hub_case(seed)
    x = np.concatenate([dummy] + songs)
    cohort = default_cohort(dummy)
    S = chain_dot(query, x)
    q_stats = cohort_stats(chain_dot(query, cohort))
    x_stats = cohort_stats(chain_dot(x, cohort))
    out = {"dummy": dummy, "songs": songs, "query": query, "x": x, "cohort": cohort, "n_dummy": dummy.shape[0],
           "song_of": np.repeat(np.arange(len(songs)), [s.shape[0] for s in songs]).astype(np.int32),
           "song_start": np.cumsum([0] + [s.shape[0] for s in songs[:-1]]),
           "S": S, "q_stats": q_stats, "x_stats": x_stats, "z": norm_cells(S, *q_stats, *x_stats)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def planted_hits(I, h):
    """of the planted query rows, how many hold their true index row (within one row) in their list I[i]; and how many hold it first"""
    a, n, song, b = HUB_PLANT
    base = h["n_dummy"] + int(h["song_start"][song])
    held = first = 0
    for t in range(n):
        true = base + b + t
        held += bool((np.abs(I[a + t] - true) <= 1).any())
        first += bool(abs(int(I[a + t][0]) - true) <= 1)
    return held, first
