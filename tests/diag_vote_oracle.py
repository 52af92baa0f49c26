"""The oracle of the diagonal-histogram vote (include/nsid.h, nsid_diag_vote), written from the rule's text in plain Python dicts:
one pair at a time, one hit at a time, every wide bin b >= 0 that can hold a hit looked at. Host only; none of the code under test is
in here."""
import numpy as np


def diag_vote_pair(I, s, L, song_of, n_dummy, exclude=-1, bin_rows=16, top=10, max_cand=4096):
    """one pair: (songs, counts, i_lo, i_hi, r_lo, r_hi) as lists of length top, and n_songs"""
    I = np.asarray(I)
    k = I.shape[1]
    B = int(bin_rows)
    empty = ([-1] * top, [0] * top, [-1] * top, [-1] * top, [-1] * top, [-1] * top)
    if L < 1 or L * k > max_cand:
        return empty + (-1,)
    n_ref = len(song_of)
    cnt = {}                                   # (song, narrow bin) -> hits
    hits = {}                                  # (song, narrow bin) -> [(i, r)]
    for j in range(L * k):
        i = s + j // k
        cid = int(I[i][j % k])
        if cid < 0 or cid < n_dummy or cid >= n_dummy + n_ref:
            continue
        r = cid - n_dummy
        c = int(song_of[r])
        if c < 0 or c == exclude:
            continue
        delta = r - (i - s) + (L - 1)
        assert delta >= 0
        n = delta // B
        cnt[(c, n)] = cnt.get((c, n), 0) + 1
        hits.setdefault((c, n), []).append((i, r))
    best = {}                                  # song -> (score, b)
    for (c, n) in cnt:
        for b in (n - 1, n):                   # the wide bins that hold narrow bin n
            if b < 0:
                continue
            w = cnt.get((c, b), 0) + cnt.get((c, b + 1), 0)
            if c not in best or w > best[c][0] or (w == best[c][0] and b < best[c][1]):
                best[c] = (w, b)
    order = sorted(best, key=lambda c: (-best[c][0], c))
    out = [list(col) for col in empty]
    for rank, c in enumerate(order[:top]):
        w, b = best[c]
        rows = hits.get((c, b), []) + hits.get((c, b + 1), [])
        assert len(rows) == w
        out[0][rank], out[1][rank] = c, w
        out[2][rank], out[3][rank] = min(i for i, _ in rows), max(i for i, _ in rows)
        out[4][rank], out[5][rank] = min(r for _, r in rows), max(r for _, r in rows)
    return tuple(out) + (len(best),)


def diag_vote(I, starts, lens, song_of, n_dummy, exclude=None, bin_rows=16, top=10):
    """all pairs: (songs, counts, i_lo, i_hi, r_lo, r_hi) int32 (pairs, top) and n_songs int32 (pairs,)"""
    res = [diag_vote_pair(I, int(s), int(L), song_of, n_dummy, -1 if exclude is None else int(exclude[p]), bin_rows, top)
           for p, (s, L) in enumerate(zip(starts, lens))]
    cols = tuple(np.asarray([r[u] for r in res], dtype=np.int32).reshape(len(res), top) for u in range(6))
    return cols + (np.asarray([r[6] for r in res], dtype=np.int32),)


def sequence_vote_pair(q, x, I, s, L, song_of, n_dummy, exclude=-1):
    """the sequence vote (include/nsid.h seq_scores + song_vote; eval.py:296-367) for one pair, on the host. x = the rows of the whole
    index (dummy ++ ref). Whichever row of the window retrieved it, candidate cid scores the mean over t < min(L, len(x) - cid) of
    q[s + t] . x[cid + t]: the candidate laid against the window's FIRST rows. The scores add up per song in walk order; the songs
    best first (stable). Returns (codes, {code: total})."""
    k = I.shape[1]
    n_ref = len(song_of)
    totals = {}
    for j in range(L * k):
        cid = int(I[s + j // k][j % k])
        if cid < 0 or cid < n_dummy or cid >= n_dummy + n_ref:
            continue
        c = int(song_of[cid - n_dummy])
        if c < 0 or c == exclude:
            continue
        m = min(L, len(x) - cid)
        score = float(np.einsum("td,td->t", q[s:s + m].astype(np.float64), x[cid:cid + m].astype(np.float64)).mean())
        totals[c] = totals.get(c, 0.0) + score
    return sorted(totals, key=lambda c: -totals[c]), totals
