"""The synthetic catalogue of the diagonal vote's end-to-end tests (test_diag_vote_cpu.py proves on the host that its expectations hold
for the rule itself; test_diag_scan_gpu.py runs it): 40 songs of 64 random unit rows, a recording of three 204-row windows of random
unit rows, one excerpt planted wholly inside window 1 and one that starts at row 150 of window 0 and crosses into window 1. Host
only."""
import numpy as np

N_SONGS, SONG_ROWS, D = 40, 64, 128
K_PROBE, WINDOW = 20, 204                     # 204 x 20 = 4080 candidates: the default window of locate / scan at k_probe = 20
NOISE = 0.5                                   # test_scan_gpu.py's PLANT_NOISE
# (recording row, song, song row, rows): 40 rows at row 120 of window 1; 60 rows from row 150 of window 0 into window 1
PLANT_INSIDE = (WINDOW + 120, 7, 10, 40)
PLANT_CROSS = (150, 23, 2, 60)
# the seed at which, for both rates, the sequence vote's first song in window 1 is not the planted one (checked in
# test_diag_vote_cpu.py::test_catalogue_planted_song_first_under_the_rule_and_not_under_the_sequence_vote)
SEED = 0
RATES = (1.0, 0.8)


def unit_rows(rng, n, d=D):
    r = rng.standard_normal((n, d))
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)


def plants(rate):
    """(recording row, song, song row, rows, rate): the inside plant at `rate`, the crossing one at 1.0"""
    return [PLANT_INSIDE + (rate,), PLANT_CROSS + (1.0,)]


def catalogue(rate, seed=SEED):
    """(songs: list of (64, 128) float32, recording (612, 128) float32); the plants as test_scan_gpu.py plants them"""
    rng = np.random.default_rng(seed)
    songs = [unit_rows(rng, SONG_ROWS) for _ in range(N_SONGS)]
    q = unit_rows(rng, 3 * WINDOW)
    for a, s, b, rows, r in plants(rate):
        for t in range(rows):
            v = songs[s][b + int(round(t * r))] + NOISE * rng.standard_normal(D) / np.sqrt(D)
            q[a + t] = (v / np.linalg.norm(v)).astype(np.float32)
    return songs, q


def brute_force_search(q, x, k):
    """the k nearest rows of x for every row of q, nearest first (fp64 L2; ties to the smaller id)"""
    d2 = ((q.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * q.astype(np.float64) @ x.astype(np.float64).T
          + (x.astype(np.float64) ** 2).sum(1)[None, :])
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)


def plant_ends(plant):
    a, s, b, rows, rate = plant
    return (a, a + rows - 1, b, b + int(round((rows - 1) * rate)))
