"""The oracle of the alignment paths (include/nsid.h nsid_align_paths): the rule of locate_oracle.py with every cell's predecessor
kept (the cell loop, and a row-vectorised form of it for the large shapes), the trace along those predecessors, the walk of an
occurrence's box alone, and the band matrices that give long paths."""
import numpy as np

from locate_oracle import DYADIC, STEPS, _shift

NONE = 0          # step codes: 0 none (a path's first cell, or a cell with H = 0), 1 = (1, 1), 2 = (1, 2), 3 = (2, 1)


def cells_from(S, theta):
    """the rule, cell by cell: (H (Lq, Lr) float32, frm (Lq, Lr) int8 step codes)"""
    S = np.asarray(S, dtype=np.float32)
    theta = np.float32(theta)
    Lq, Lr = S.shape
    H = np.zeros((Lq, Lr), dtype=np.float32)
    frm = np.zeros((Lq, Lr), dtype=np.int8)
    for i in range(Lq):
        for j in range(Lr):
            e = np.float32(S[i, j] - theta)
            best, code = np.float32(0), NONE
            for c, (di, dj) in enumerate(STEPS, start=1):
                a, b = i - di, j - dj
                if a >= 0 and b >= 0 and H[a, b] > best:
                    best, code = H[a, b], c
            v = np.float32(best + e)
            if v > 0:
                H[i, j] = v
                frm[i, j] = code
    return H, frm


def rows_from(S, theta):
    """the same a row at a time: (H, frm)"""
    S = np.asarray(S, dtype=np.float32)
    theta = np.float32(theta)
    Lq, Lr = S.shape
    H = np.zeros((Lq, Lr), dtype=np.float32)
    frm = np.zeros((Lq, Lr), dtype=np.int8)
    zero = np.zeros(Lr, dtype=np.float32)
    h1, h2 = zero, zero                                       # rows i - 1 and i - 2
    for i in range(Lq):
        e = (S[i] - theta).astype(np.float32)
        best = np.zeros(Lr, dtype=np.float32)
        code = np.zeros(Lr, dtype=np.int8)
        for c, hp in enumerate((_shift(h1, 1, 0), _shift(h1, 2, 0), _shift(h2, 1, 0)), start=1):
            take = hp > best
            best = np.where(take, hp, best)
            code = np.where(take, np.int8(c), code)
        v = (best + e).astype(np.float32)
        pos = v > 0
        H[i] = np.where(pos, v, np.float32(0))
        frm[i] = np.where(pos, code, np.int8(NONE))
        h2, h1 = h1, H[i]
    return H, frm


def trace(frm, i, j):
    """the path that ends at cell (i, j), which has H > 0: (rows, columns) int32 arrays in forward order"""
    cells = []
    while True:
        cells.append((i, j))
        c = int(frm[i, j])
        if c == NONE:
            break
        di, dj = STEPS[c - 1]
        i, j = i - di, j - dj
    cells.reverse()
    a = np.asarray(cells, dtype=np.int32)
    return a[:, 0].copy(), a[:, 1].copy()


def box_path(S, theta, i0, i1, j0, j1, form=rows_from):
    """the rule on the box S[i0..i1][j0..j1] alone and the trace from its last cell: (rows, columns, last H) in the coordinates of S,
    or (None, None, last H) when the last H is not positive or the trace does not end at the box's first cell"""
    H, frm = form(np.asarray(S, dtype=np.float32)[i0:i1 + 1, j0:j1 + 1], theta)
    if not H[-1, -1] > 0:
        return None, None, H[-1, -1]
    pi, pj = trace(frm, i1 - i0, j1 - j0)
    if pi[0] != 0 or pj[0] != 0:
        return None, None, H[-1, -1]
    return pi + np.int32(i0), pj + np.int32(j0), H[-1, -1]


def band(rng, n_rows, n_cols, rate, half=3):
    """dyadic values within `half` columns of the line j = round(rate i), 0 elsewhere: long paths in a wide matrix"""
    S = np.zeros((n_rows, n_cols), dtype=np.float32)
    mid = np.rint(rate * np.arange(n_rows)).astype(np.int64)
    for d in range(-half, half + 1):
        j = mid + d
        ok = (j >= 0) & (j < n_cols)
        S[np.nonzero(ok)[0], j[ok]] = DYADIC[rng.integers(0, DYADIC.size, size=int(ok.sum()))]
    return S


def spans(n_rows, n_cols):
    """can one path go from the first to the last cell of an n_rows x n_cols box? (every step advances each index by 1 or 2)"""
    dr, dc = n_rows - 1, n_cols - 1
    return dr >= 0 and dc >= 0 and dr <= 2 * dc and dc <= 2 * dr


def spanning_band(rng, n_rows, n_cols, half=3, clear=4):
    """A band matrix that is one occurrence's box, so that a test chooses the box's sides: the band around the line from the first
    cell to the last one (rate (n_cols - 1) / (n_rows - 1)), on it a chain of cells of 1.0 from corner to corner by steps of the rule,
    and nothing but the chain in the first `clear` rows and columns, so that no other path starts beside the chain's. That the last
    cell's path does start at the first cell is for the oracle to say (box_path); the tests assert it."""
    assert spans(n_rows, n_cols)
    dr, dc = n_rows - 1, n_cols - 1
    S = band(rng, n_rows, n_cols, dc / dr if dr else 1.0, half)
    S[:clear] = 0
    S[:, :clear] = 0
    i = j = 0
    S[0, 0] = 1.0
    while (i, j) != (dr, dc):
        best = None
        for di, dj in STEPS:
            a, b = i + di, j + dj
            if not spans(n_rows - a, n_cols - b):
                continue
            dev = abs(b * dr - a * dc)                        # the distance from the line, up to a factor
            if best is None or dev < best[0]:
                best = (dev, a, b)
        _, i, j = best
        S[i, j] = 1.0
    return S


def line(q_rows, r_rows):
    """(slope, intercept) of the fp64 least-squares line of song row over query row (np.polyfit, as the issue's figures were made)"""
    a, b = np.polyfit(np.asarray(q_rows, dtype=np.float64), np.asarray(r_rows, dtype=np.float64), 1)
    return float(a), float(b)
