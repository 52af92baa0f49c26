"""The oracle of the scan (include/nsid.h, below nsid_local_align): the alignment rule a row at a time from carried rows to carried
rows, with unpacked global origins (locate_oracle.align_rows with a carry), the occurrences of a run of rows grouped by (i0, j0), and
the active-set and run rule of SampleIndex.scanner replayed from per-window votes and open_h values. Host only; none of the code under
test is in here."""
import numpy as np


def fresh_carry(Lr):
    """rows -1 and -2 as 'H = +0, no origin': (h (2, Lr) float32, i0 (2, Lr) int32, j0 (2, Lr) int32); index 0 = row i - 1"""
    return np.zeros((2, Lr), np.float32), np.full((2, Lr), -1, np.int32), np.full((2, Lr), -1, np.int32)


def _shift(row, n, fill):
    out = np.full_like(row, fill)
    if n < row.size:
        out[n:] = row[: row.size - n]
    return out


def align_strip(S, theta, row_base, carry):
    """one strip: S (n, Lr) are the global rows row_base .. row_base + n - 1. Returns (row_h, row_j, row_i0, row_j0, carry out, open_h);
    the carry out is the last two rows of (old row -2, old row -1, the strip's rows)"""
    S = np.asarray(S, dtype=np.float32)
    theta = np.float32(theta)
    n, Lr = S.shape
    ch, ci, cj = carry
    h1, i1, j1, h2, i2, j2 = ch[0], ci[0], cj[0], ch[1], ci[1], cj[1]
    cols = np.arange(Lr, dtype=np.int32)
    row_h = np.zeros(n, dtype=np.float32)
    row_j = np.full(n, -1, dtype=np.int32)
    row_i0 = np.full(n, -1, dtype=np.int32)
    row_j0 = np.full(n, -1, dtype=np.int32)
    for r in range(n):
        e = (S[r] - theta).astype(np.float32)
        best = np.zeros(Lr, dtype=np.float32)
        fi = np.full(Lr, -1, dtype=np.int32)
        fj = np.full(Lr, -1, dtype=np.int32)
        for hp, ip, jp in ((_shift(h1, 1, 0), _shift(i1, 1, -1), _shift(j1, 1, -1)), (_shift(h1, 2, 0), _shift(i1, 2, -1), _shift(j1, 2, -1)),
                           (_shift(h2, 1, 0), _shift(i2, 1, -1), _shift(j2, 1, -1))):
            take = hp > best
            best = np.where(take, hp, best)
            fi = np.where(take, ip, fi)
            fj = np.where(take, jp, fj)
        with np.errstate(invalid="ignore"):
            v = (best + e).astype(np.float32)
            pos = v > 0
            h = np.where(pos, v, np.float32(0)).astype(np.float32)
            oi = np.where(pos, np.where(fi >= 0, fi, np.int32(row_base + r)), -1).astype(np.int32)
            oj = np.where(pos, np.where(fi >= 0, fj, cols), -1).astype(np.int32)
            ok = e > 0
        if ok.any():
            j = int(np.argmax(np.where(ok, h, np.float32(-1))))          # the first of the largest: ties to the smallest j
            row_h[r], row_j[r], row_i0[r], row_j0[r] = h[j], j, oi[j], oj[j]
        h2, i2, j2, h1, i1, j1 = h1, i1, j1, h, oi, oj
    out = (np.stack([h1, h2]).astype(np.float32), np.stack([i1, i2]).astype(np.int32), np.stack([j1, j2]).astype(np.int32))
    return row_h, row_j, row_i0, row_j0, out, np.float32(max(float(out[0].max()) if Lr else 0.0, 0.0))


def align_chained(S, theta, cuts, row_base=0):
    """the strips of `cuts` rows chained over S from a fresh carry: (row_h, row_j, row_i0, row_j0) of all rows, the carry after the last
    strip, and the open_h after every strip"""
    S = np.asarray(S, dtype=np.float32)
    assert sum(cuts) == S.shape[0]
    carry = fresh_carry(S.shape[1])
    parts, opens, lo = [], [], 0
    for n in cuts:
        *rows, carry, oh = align_strip(S[lo:lo + n], theta, row_base + lo, carry)
        parts.append(rows)
        opens.append(oh)
        lo += n
    cat = [np.concatenate([p[u] for p in parts]) if parts else np.zeros(0) for u in range(4)]
    return cat[0].astype(np.float32), cat[1].astype(np.int32), cat[2].astype(np.int32), cat[3].astype(np.int32), carry, opens


def rows_from_cells(S, theta, H, org, row_base=0):
    """the row results of the whole matrix from locate_oracle.align_cells' H and packed org (i0 << 16 | j0, rows local), unpacked and
    moved to global rows"""
    S = np.asarray(S, dtype=np.float32)
    Lq, Lr = S.shape
    row_h = np.zeros(Lq, dtype=np.float32)
    row_j = np.full(Lq, -1, dtype=np.int32)
    row_i0 = np.full(Lq, -1, dtype=np.int32)
    row_j0 = np.full(Lq, -1, dtype=np.int32)
    for i in range(Lq):
        for j in range(Lr):
            if np.float32(S[i, j] - np.float32(theta)) > 0 and H[i, j] > row_h[i]:
                row_h[i], row_j[i] = H[i, j], j
                row_i0[i], row_j0[i] = (int(org[i, j]) >> 16) + row_base, int(org[i, j]) & 0xffff
    return row_h, row_j, row_i0, row_j0


def occurrences_unpacked(row_h, row_j, row_i0, row_j0, first_row=0, min_score=0.0, top=16):
    """(occ (top, 4) int32 = (i0, i1 = first_row + local row, j0, j1), occ_score (top,) float32, n_occ) of one run of rows"""
    groups = {}
    for i in range(len(row_h)):
        if row_i0[i] < 0:
            continue
        g = (int(row_i0[i]), int(row_j0[i]))
        if g not in groups or row_h[i] > row_h[groups[g]]:           # ties to the smallest i: the first stays
            groups[g] = i
    kept = [(g, i) for g, i in groups.items() if row_h[i] >= np.float32(min_score)]
    kept.sort(key=lambda t: (-float(row_h[t[1]]), t[0][0], t[0][1]))
    occ = np.full((top, 4), -1, dtype=np.int32)
    sc = np.zeros(top, dtype=np.float32)
    for n, (g, i) in enumerate(kept[:top]):
        occ[n] = (g[0], first_row + i, g[1], row_j[i])
        sc[n] = row_h[i]
    return occ, sc, len(kept)


def replay_active(votes, opens, n_songs, max_active):
    """The active-set rule. votes[t]: the song codes of window t's vote, best first; opens[t]: {code: open_h} of the songs that were
    active in window t (what the strips left). Returns (active[t] lists, closed_at_cap, runs = [(code, first window, last window)]).
    Window t: the songs active in t - 1 with open_h > 0, by open_h descending, then code; then the vote's first n_songs songs that are
    not among them, in vote order; cut at max_active (the songs cut are counted). A run is a maximal stretch of consecutive windows."""
    active, closed, prev = [], 0, []
    for t, vote in enumerate(votes):
        cont = sorted((c for c in prev if opens[t - 1][c] > 0), key=lambda c: (-opens[t - 1][c], c))
        want = cont + [c for c in list(vote)[:n_songs] if c not in cont]
        closed += max(0, len(want) - max_active)
        want = want[:max_active]
        active.append(want)
        prev = want
    runs, open_run = [], {}
    for t, want in enumerate(active):
        for c in list(open_run):
            if c not in want:
                runs.append((c, open_run.pop(c), t - 1))
        for c in want:
            open_run.setdefault(c, t)
    runs += [(c, t0, len(active) - 1) for c, t0 in open_run.items()]
    return active, closed, sorted(runs, key=lambda r: (r[1], r[0]))
