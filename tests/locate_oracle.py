"""The oracle of the local alignment (include/nsid.h, "locating a sample"): the rule as a cell loop, a row-vectorised numpy form of
it (shown equal to the loop in test_locate_cpu.py; the GPU tests use it at the large shapes), the occurrences, and the generator of
planted cases."""
import numpy as np

DYADIC = np.array([0.0, 0.25, -0.25, 0.375, 0.5, 0.625, 0.75, 1.0], dtype=np.float32)     # exact ties abound
STEPS = ((1, 1), (1, 2), (2, 1))


def dyadic(rng, Lq, Lr):
    return DYADIC[rng.integers(0, DYADIC.size, size=(Lq, Lr))]


def align_cells(S, theta):
    """the rule, cell by cell: (H (Lq, Lr) float32, org (Lq, Lr) int32 = i0 << 16 | j0, -1 = none)"""
    S = np.asarray(S, dtype=np.float32)
    theta = np.float32(theta)
    Lq, Lr = S.shape
    H = np.zeros((Lq, Lr), dtype=np.float32)
    org = np.full((Lq, Lr), -1, dtype=np.int32)
    for i in range(Lq):
        for j in range(Lr):
            e = np.float32(S[i, j] - theta)
            best, frm = np.float32(0), None
            for di, dj in STEPS:
                a, b = i - di, j - dj
                if a >= 0 and b >= 0 and H[a, b] > best:
                    best, frm = H[a, b], (a, b)
            v = np.float32(best + e)
            if v > 0:
                H[i, j] = v
                org[i, j] = org[frm] if frm is not None else (i << 16 | j)
    return H, org


def _shift(row, n, fill):
    out = np.full_like(row, fill)
    if n < row.size:
        out[n:] = row[: row.size - n]
    return out


def align_rows(S, theta, want_cells=False):
    """the same rule a row at a time; returns (row_h, row_j, row_org) and, with want_cells, also (H, org)"""
    S = np.asarray(S, dtype=np.float32)
    theta = np.float32(theta)
    Lq, Lr = S.shape
    zero_h, none = np.zeros(Lr, dtype=np.float32), np.full(Lr, -1, dtype=np.int32)
    h1, o1, h2, o2 = zero_h, none, zero_h, none               # rows i - 1 and i - 2
    cols = np.arange(Lr, dtype=np.int32)
    row_h = np.zeros(Lq, dtype=np.float32)
    row_j = np.full(Lq, -1, dtype=np.int32)
    row_org = np.full(Lq, -1, dtype=np.int32)
    Hs, Os = [], []
    for i in range(Lq):
        e = (S[i] - theta).astype(np.float32)
        best = np.zeros(Lr, dtype=np.float32)
        frm = np.full(Lr, -1, dtype=np.int32)
        for hp, op in ((_shift(h1, 1, 0), _shift(o1, 1, -1)), (_shift(h1, 2, 0), _shift(o1, 2, -1)), (_shift(h2, 1, 0), _shift(o2, 1, -1))):
            take = hp > best
            best = np.where(take, hp, best)
            frm = np.where(take, op, frm)
        with np.errstate(invalid="ignore"):
            v = (best + e).astype(np.float32)
            pos = v > 0
            h = np.where(pos, v, np.float32(0)).astype(np.float32)
            o = np.where(pos, np.where(frm >= 0, frm, (np.int32(i) << 16) | cols), -1).astype(np.int32)
            ok = e > 0
        if ok.any():
            hv = np.where(ok, h, np.float32(-1))
            j = int(np.argmax(hv))                            # the first of the largest: ties to the smallest j
            row_h[i], row_j[i], row_org[i] = h[j], j, o[j]
        if want_cells:
            Hs.append(h)
            Os.append(o)
        h2, o2, h1, o1 = h1, o1, h, o
    if want_cells:
        return row_h, row_j, row_org, np.stack(Hs) if Hs else np.zeros((0, Lr), np.float32), np.stack(Os) if Os else np.zeros((0, Lr), np.int32)
    return row_h, row_j, row_org


def row_results_from_cells(S, theta, H, org):
    """the row results of the rule from the cell loop's H and org (the plain statement, for the comparison with align_rows)"""
    S = np.asarray(S, dtype=np.float32)
    Lq, Lr = S.shape
    row_h = np.zeros(Lq, dtype=np.float32)
    row_j = np.full(Lq, -1, dtype=np.int32)
    row_org = np.full(Lq, -1, dtype=np.int32)
    for i in range(Lq):
        for j in range(Lr):
            if np.float32(S[i, j] - np.float32(theta)) > 0 and H[i, j] > row_h[i]:
                row_h[i], row_j[i], row_org[i] = H[i, j], j, org[i, j]
    return row_h, row_j, row_org


def occurrences(row_h, row_j, row_org, min_score=0.0, top=16):
    """(occ (top, 4) int32, occ_score (top,) float32, n_occ) of one pair"""
    groups = {}
    for i in range(row_h.size):
        g = int(row_org[i])
        if g == -1:
            continue
        if g not in groups or row_h[i] > row_h[groups[g]]:     # ties to the smallest i: the first stays
            groups[g] = i
    kept = [(g, i) for g, i in groups.items() if row_h[i] >= np.float32(min_score)]
    kept.sort(key=lambda t: (-float(row_h[t[1]]), t[0] >> 16, t[0] & 0xffff))
    occ = np.full((top, 4), -1, dtype=np.int32)
    sc = np.zeros(top, dtype=np.float32)
    for n, (g, i) in enumerate(kept[:top]):
        occ[n] = (g >> 16, i, g & 0xffff, row_j[i])
        sc[n] = row_h[i]
    return occ, sc, len(kept)


def align_oracle(S, theta, min_score=0.0, top=16):
    """everything local_align returns for one pair: (occ, occ_score, n_occ, row_h, row_j, row_org)"""
    S = np.asarray(S, dtype=np.float32)
    if S.shape[0] == 0 or S.shape[1] == 0:                   # rows without a column have no cell: 0, -1, -1
        n = S.shape[0]
        e = np.zeros(n, dtype=np.float32), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        return (np.full((top, 4), -1, dtype=np.int32), np.zeros(top, dtype=np.float32), 0) + e
    rows = align_rows(S, theta)
    return occurrences(*rows, min_score, top) + rows


def smooth_rows(rng, n, d, w=8):
    """overlapping segments: neighbouring rows correlate"""
    f = rng.standard_normal((n + w - 1, d))
    r = np.stack([f[t:t + w].sum(0) for t in range(n)])
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)


def case(seed, Lq, Lr, d, plants, noise):
    """plants: (query row a, song row b, rows n, rate)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = smooth_rows(rng, Lr, d)
    q = smooth_rows(rng, Lq, d)
    for a, b, n, rate in plants:
        for t in range(n):
            v = ref[b + int(round(t * rate))] + noise * rng.standard_normal(d) / np.sqrt(d)
            q[a + t] = (v / np.linalg.norm(v)).astype(np.float32)
    return q, ref


PLANT_SHAPE = (100, 90, 128)
PLANTS = [(5, 20, 12, 1.0), (30, 60, 16, 0.75), (60, 10, 10, 1.5), (80, 20, 12, 1.0)]
PLANT_NOISE, PLANT_THETA, PLANT_MIN_SCORE = 0.5, 0.6, 2.0
PLANT_SEEDS = range(6)


def plants_matched(occ, n_occ, plants=PLANTS):
    """the issue's condition: exactly len(plants) occurrences, and each plant is matched by exactly one of them with all four ends
    within one row"""
    if n_occ != len(plants):
        return False
    for a, b, n, rate in plants:
        want = (a, a + n - 1, b, b + int(round((n - 1) * rate)))
        hits = [o for o in occ[:n_occ].tolist() if all(abs(o[u] - want[u]) <= 1 for u in range(4))]
        if len(hits) != 1:
            return False
    return True
