"""The oracle of the cohort score normalisation (include/nsid.h, "cohort score normalisation"): pair_sim's dot as an exact fp32 fma
chain, the two fp64 sums in the header's order, mu and rs, the normalised cell with its five separate fp32 roundings, and the
generator of the hub case. The alignment itself is locate_oracle's, the strips scan_oracle's and the paths align_path_oracle's:
nothing of them is restated here."""
import numpy as np

import align_path_oracle
import locate_oracle
import scan_oracle
from locate_oracle import align_oracle, smooth_rows

CHUNK, CLASSES = 256, 32          # NSID_COHORT_CHUNK, the column classes of a chunk
VAR_FLOOR = 1e-12

box_path = align_path_oracle.box_path          # the three oracles this one builds on, under the names the tests use
align_chained, occurrences_unpacked = scan_oracle.align_chained, scan_oracle.occurrences_unpacked
occurrences = locate_oracle.occurrences


# ---------------------------------------------------------------------------------------------------- pair_sim's dot
def fma32(a, b, c):
    """fp32 fma(a, b, c), exactly: the product is exact in fp64, the sum is rounded to odd there (TwoSum gives its error), and 53 bits
    rounded to odd round to 24 bits as the exact sum does"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0)
    bits[fix] += np.where((err[fix] > 0) == (s[fix] > 0), 1, -1)          # one ulp towards the exact sum: in magnitude, up or down
    return bits.view(np.float64).astype(np.float32)


def chain_order(d):
    """the k order of pair_sim's chain: up to d = 256 step (b, e) takes k = 8 b + e and then k = 8 b + 4 + e, above it k ascends"""
    if d > 256:
        return np.arange(d)
    return (8 * np.arange(d // 8)[:, None] + np.array([0, 4, 1, 5, 2, 6, 3, 7])[None, :]).reshape(-1)


def chain_dot(q, x):
    """S[i, j] = q[i] . x[j] as pair_sim forms it: one k-ordered fp32 fma chain from +0"""
    q, x = np.asarray(q, dtype=np.float32), np.asarray(x, dtype=np.float32)
    acc = np.zeros((q.shape[0], x.shape[0]), dtype=np.float32)
    for k in chain_order(q.shape[1]):
        acc = fma32(np.broadcast_to(q[:, k, None], acc.shape), np.broadcast_to(x[None, :, k], acc.shape), acc)
    return acc


# ---------------------------------------------------------------------------------------------------- the statistics
def _ordered(t):
    """the fp64 sum of every row of t (n, M) in the header's order"""
    n, M = t.shape
    flip = [np.arange(CLASSES) ^ dist for dist in (1, 2, 4, 8, 16)]
    total = None
    for c0 in range(0, M, CHUNK):
        blk = t[:, c0:c0 + CHUNK]
        a = np.zeros((n, CLASSES), dtype=np.float64)
        for t0 in range(0, blk.shape[1], CLASSES):              # class r = m mod 32, ascending m
            tile = blk[:, t0:t0 + CLASSES]
            a[:, :tile.shape[1]] += tile
        for f in flip:                                          # a[r] += a[r ^ dist], all r at once
            a = a + a[:, f]
        total = a[:, 0].copy() if total is None else total + a[:, 0]
    return total


def ordered_sums(s):
    """s (n, M) fp32 scores against the cohort -> (A, B) fp64: the sum and the sum of squares (a square is exact in fp64)"""
    s64 = np.asarray(s, dtype=np.float32).astype(np.float64)
    return _ordered(s64), _ordered(s64 * s64)


def stats_from_sums(A, B, M):
    mu64 = A / np.float64(M)
    var64 = np.maximum(B / np.float64(M) - mu64 * mu64, VAR_FLOOR)
    return mu64.astype(np.float32), (1.0 / np.sqrt(var64)).astype(np.float32)


def cohort_stats(s):
    """(mu, rs) fp32 of every row from its scores s (n, M) against the cohort"""
    return stats_from_sums(*ordered_sums(s), np.asarray(s).shape[1])


def norm_cells(S, q_mu, q_rs, x_mu, x_rs):
    """S' = 0.5 ((S - q_mu[i]) q_rs[i] + (S - x_mu[j]) x_rs[j]): five fp32 operations, each rounded once"""
    S = np.asarray(S, dtype=np.float32)
    q_mu, q_rs, x_mu, x_rs = (np.asarray(v, dtype=np.float32) for v in (q_mu, q_rs, x_mu, x_rs))
    zq = ((S - q_mu[:, None]).astype(np.float32) * q_rs[:, None]).astype(np.float32)
    zx = ((S - x_mu[None, :]).astype(np.float32) * x_rs[None, :]).astype(np.float32)
    return (np.float32(0.5) * (zq + zx).astype(np.float32)).astype(np.float32)


def normalised(q, x, cohort, dot=chain_dot):
    """(S', S) of query rows q against song rows x under the cohort, everything in the oracle's own arithmetic"""
    S = dot(q, x)
    return norm_cells(S, *cohort_stats(dot(q, cohort)), *cohort_stats(dot(x, cohort))), S


# ---------------------------------------------------------------------------------------------------- the hub case
HUB_SHAPE = (100, 90, 128)
HUB_PLANTS = [(5, 20, 12, 1.0), (30, 60, 16, 0.75), (80, 20, 12, 1.0)]
HUB_NOISE = 0.5
HUB_Q, HUB_R = (50, 69), (35, 54)               # the generic stretch: query rows, song rows (inclusive)
HUB_COHORT, HUB_COHORT_SHARE = 512, 0.15
HUB_SEEDS = range(6)
RAW_THETA, RAW_MIN_SCORE = 0.6, 2.0
NORM_THETA, NORM_MIN_SCORE = 7.0, 10.0


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def hub_case(seed):
    """(query, song, cohort) fp32 rows. Drawn from one PCG64 generator in this order: u, song, query, plants, query hubs, song hubs,
    cohort, cohort hubs. A generic row is unit(2 u + g / sqrt(d)), g standard normal."""
    Lq, Lr, d = HUB_SHAPE
    rng = np.random.Generator(np.random.PCG64(seed))
    u = _unit(rng.standard_normal(d)).astype(np.float64)

    def generic(n):
        return _unit(2.0 * u[None, :] + rng.standard_normal((n, d)) / np.sqrt(d))

    song = smooth_rows(rng, Lr, d)
    query = smooth_rows(rng, Lq, d)
    for a, b, n, rate in HUB_PLANTS:
        for t in range(n):
            query[a + t] = _unit(song[b + int(round(t * rate))] + HUB_NOISE * rng.standard_normal(d) / np.sqrt(d))
    query[HUB_Q[0]:HUB_Q[1] + 1] = generic(HUB_Q[1] - HUB_Q[0] + 1)
    song[HUB_R[0]:HUB_R[1] + 1] = generic(HUB_R[1] - HUB_R[0] + 1)
    cohort = smooth_rows(rng, HUB_COHORT, d)
    which = rng.choice(HUB_COHORT, size=int(round(HUB_COHORT_SHARE * HUB_COHORT)), replace=False)
    cohort[which] = generic(which.size)
    return query, song, cohort


def plants_found(occ, n_occ, plants=HUB_PLANTS):
    """every plant is matched by exactly one occurrence with all four ends within one row"""
    rows = occ[:min(int(n_occ), len(occ))].tolist()
    for a, b, n, rate in plants:
        want = (a, a + n - 1, b, b + int(round((n - 1) * rate)))
        if sum(all(abs(o[u] - want[u]) <= 1 for u in range(4)) for o in rows) != 1:
            return False
    return True


def in_box(occ, n_occ):
    """the occurrences that overlap the box of generic query rows x generic song rows"""
    return [o for o in occ[:min(int(n_occ), len(occ))].tolist()
            if o[0] <= HUB_Q[1] and o[1] >= HUB_Q[0] and o[2] <= HUB_R[1] and o[3] >= HUB_R[0]]


def hub_condition(S_raw, S_norm, top=16):
    """the issue's condition on one seed: (raw plants found, raw occurrences in the box, normalised plants found, normalised in the box)"""
    raw = align_oracle(S_raw, RAW_THETA, RAW_MIN_SCORE, top)
    nrm = align_oracle(S_norm, NORM_THETA, NORM_MIN_SCORE, top)
    return plants_found(raw[0], raw[2]), len(in_box(raw[0], raw[2])), plants_found(nrm[0], nrm[2]), len(in_box(nrm[0], nrm[2]))
