"""CPU: the diagonal-histogram vote's rule (diag_vote_oracle.py) on hand-made tables whose answers are written out here, the synthetic
catalogue of test_diag_scan_gpu.py under the rule and under the sequence vote (brute-force search in numpy), and the new entry's
binding, limits and keyword refusals without a launch."""
import numpy as np
import pytest

import diag_scan_case as C
from diag_vote_oracle import diag_vote, diag_vote_pair, sequence_vote_pair


def _pair(I, s, L, song_of, n_dummy=0, exclude=-1, bin_rows=4, top=3):
    return diag_vote_pair(np.asarray(I, dtype=np.int64), s, L, song_of, n_dummy, exclude, bin_rows, top)


# ---- the rule by hand: delta = r - (i - s) + (L - 1), narrow bin = delta // B

def test_tie_between_two_songs_goes_to_the_smaller_code():
    song_of = [0] * 8 + [1] * 8
    # song 1 is walked first: r = 8, 9 at rows 0, 1 -> delta 9, 9 (bin 2); song 0: r = 0, 1 -> delta 1, 1 (bin 0). 2 hits each
    got = _pair([[8, 0], [9, 1]], 0, 2, song_of)
    assert got == ([0, 1, -1], [2, 2, 0], [0, 0, -1], [1, 1, -1], [0, 8, -1], [1, 9, -1], 2)


def test_tie_between_two_bins_of_a_song_goes_to_the_smaller_bin():
    # delta 1, 1 (bin 0) and 21, 21 (bin 5): wide[0] = 2, wide[4] = wide[5] = 2 -> b = 0: the rows of the first two hits
    got = _pair([[20, 0], [21, 1]], 0, 2, [0] * 32)
    assert got == ([0, -1, -1], [2, 0, 0], [0, -1, -1], [1, -1, -1], [0, -1, -1], [1, -1, -1], 1)
    # three hits in bin 5 against two in bin 0: the larger bin wins whatever its place
    got = _pair([[20, 0], [21, 1], [22, -1]], 0, 3, [0] * 32)          # delta 22, 22, 22 (bin 5) and 2, 2 (bin 0)
    assert got == ([0, -1, -1], [3, 0, 0], [0, -1, -1], [2, -1, -1], [20, -1, -1], [22, -1, -1], 1)


def test_a_diagonal_across_a_narrow_bin_edge_is_counted_whole():
    # song 0 at twice the speed: r = 3, 5, 7, 9 at rows 0 .. 3 -> delta 6, 7, 8, 9 = bins 1, 1, 2, 2: wide[1] = 4.
    # song 1: r = 16, 17, 18 at rows 0 .. 2 -> delta 19, 19, 19 = bin 4: 3 hits. Narrow bins alone would rank song 1 (3) over song 0 (2)
    song_of = [0] * 16 + [1] * 16
    got = _pair([[3, 16], [5, 17], [7, 18], [9, -1]], 0, 4, song_of)
    assert got == ([0, 1, -1], [4, 3, 0], [0, 0, -1], [3, 2, -1], [3, 16, -1], [9, 18, -1], 2)


def test_a_repeated_candidate_counts_again_and_rows_are_table_rows():
    # the pair is row 2 alone (s = 2, L = 1): i_lo / i_hi are indices into the table, delta = r
    got = _pair([[1, 1], [2, 2], [5, 5]], 2, 1, [0] * 8)
    assert got == ([0, -1, -1], [2, 0, 0], [2, -1, -1], [2, -1, -1], [5, -1, -1], [5, -1, -1], 1)


def test_every_skip_condition():
    song_of = [0, 0, -1, 1, 1, 2]                                       # n_dummy = 3: ids 3 .. 8 are ref rows 0 .. 5
    row = [[-1, 2, 9, 5, 6, 3, 8]]       # the -1 tail, a dummy id, an id past n_dummy + n_ref, a row that never votes, song 1, song 0, song 2
    got = _pair(row, 0, 1, song_of, n_dummy=3, exclude=1, bin_rows=16)
    assert got == ([0, 2, -1], [1, 1, 0], [0, 0, -1], [0, 0, -1], [0, 5, -1], [0, 5, -1], 2)
    got = _pair(row, 0, 1, song_of, n_dummy=3, exclude=-1, bin_rows=16)
    assert got == ([0, 1, 2], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 3, 5], [0, 3, 5], 3)
    got = _pair(row, 0, 1, song_of, n_dummy=3, exclude=-1, bin_rows=16, top=2)          # more songs than top
    assert got == ([0, 1], [1, 1], [0, 0], [0, 0], [0, 3], [0, 3], 3)


def test_a_pair_past_the_candidate_limit_is_an_empty_row():
    I = np.zeros((4097, 1), dtype=np.int64)
    assert _pair(I, 0, 4097, [0]) == ([-1] * 3, [0] * 3, [-1] * 3, [-1] * 3, [-1] * 3, [-1] * 3, -1)
    assert _pair(I, 0, 0, [0])[6] == -1
    # 4096 rows that all retrieve ref row 0: delta = 4095 - i, 16 per narrow bin, 32 per wide bin; b = 0 holds the last 32 rows
    cols = diag_vote(I, [0, 0], [4097, 4096], [0], 0, None, 16, 2)
    assert cols[0].tolist() == [[-1, -1], [0, -1]] and cols[1].tolist() == [[0, 0], [32, 0]] and cols[6].tolist() == [-1, 1]
    assert cols[2].tolist() == [[-1, -1], [4064, -1]] and cols[3].tolist() == [[-1, -1], [4095, -1]]
    assert all(c.dtype == np.int32 for c in cols)


# ---- the catalogue of the end-to-end GPU test, on the host

@pytest.mark.parametrize("rate", C.RATES)
def test_catalogue_planted_song_first_under_the_rule_and_not_under_the_sequence_vote(rate):
    """What test_diag_scan_gpu.py expects of the GPU holds for the rule itself: in the plant's window the planted song is the diagonal
    vote's first song with at least the plant's rows as its count, and the sequence vote (candidates laid against the window's first
    rows) does not put it in its first n_songs = 1. Recorded at diag_scan_case.SEED = 0: counts 61 (inside plant, both rates) and 68
    (crossing plant, 54 of its rows in window 0); the sequence vote ranks the inside plant's song 13th (rate 1.0) and 5th (0.8)."""
    songs, q = C.catalogue(rate)
    x = np.concatenate(songs)
    song_of = np.repeat(np.arange(C.N_SONGS), C.SONG_ROWS).astype(np.int32)
    I = C.brute_force_search(q, x, C.K_PROBE)
    inside, cross = C.plants(rate)
    for plant, window in ((cross, 0), (inside, 1)):
        a, s, b, rows, r = plant
        in_window = min(a + rows, (window + 1) * C.WINDOW) - a
        got = diag_vote_pair(I, window * C.WINDOW, C.WINDOW, song_of, 0, -1, 16, 3)
        assert got[0][0] == s and got[1][0] >= in_window, (plant, got)
        lo, hi = max(a, window * C.WINDOW), min(a + rows, (window + 1) * C.WINDOW) - 1
        assert got[2][0] <= lo + 1 and got[3][0] >= hi - 1                       # the hint spans the plant's rows in the window
        assert got[1][1] < got[1][0] // 2 + 5                                    # and no other song comes close
    order, _ = sequence_vote_pair(q, x, I, C.WINDOW, C.WINDOW, song_of, 0)
    assert inside[1] not in order[:1], order[:5]


# ---- the entry, its binding and the refusals that need no launch

def test_header_binding_and_limits_of_the_entry():
    from neuralsampleid_amd import _lib, ops
    assert _lib.SIGNATURES["nsid_diag_vote"] == "pippipiipiippppppps"
    assert "nsid_diag_vote" in _lib.EXPORTS and "diag_vote" in ops.launch_counters()
    assert ops.DIAG_MAX_BIN == _lib.DEFINES["NSID_DIAG_MAX_BIN"] == 4096
    lib, N = _lib.lib, None
    _lib.launch_counters(reset=True)
    call = lambda k=1, n_ref=0, n_dummy=0, B=16, top=1, npairs=0: lib.nsid_diag_vote(N, k, N, N, npairs, N, n_ref, n_dummy, N, B, top,
                                                                                      N, N, N, N, N, N, N, N)
    assert call() == 0
    for kw, rc in ((dict(k=ops.SEARCH_MAX_K), 0), (dict(k=ops.SEARCH_MAX_K + 1), -1), (dict(k=0), -1),
                   (dict(top=ops.VOTE_MAX_TOP), 0), (dict(top=ops.VOTE_MAX_TOP + 1), -1), (dict(top=0), -1),
                   (dict(B=1), 0), (dict(B=4096), 0), (dict(B=0), -1), (dict(B=4097), -1),
                   (dict(n_ref=2 ** 31 - 4097), 0), (dict(n_ref=2 ** 31 - 4096), -1), (dict(n_dummy=-1), -1), (dict(npairs=-1), -1),
                   (dict(npairs=1), -1)):                                       # a pair, and null tables
        assert call(**kw) == rc, kw
    assert sum(_lib.launch_counters().values()) == 0


def test_vote_keyword_refusals_come_before_the_device():
    from neuralsampleid_amd.identify import SampleIndex, _vote_options
    assert _vote_options("x", "sequence", 16, 2, rerank=True) == ("sequence", 16, 2)
    assert _vote_options("x", "diagonal", 4096, 1) == ("diagonal", 4096, 1)
    for bad in (dict(vote="histogram"), dict(vote=None), dict(vote="diagonal", rerank=True), dict(vote="diagonal", bin_rows=0),
                dict(vote="diagonal", bin_rows=4097), dict(vote="diagonal", min_hits=0)):
        kw = dict(vote="diagonal", bin_rows=16, min_hits=2, rerank=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            _vote_options("x", kw["vote"], kw["bin_rows"], kw["min_hits"], kw["rerank"])
    idx = SampleIndex(None)
    with pytest.raises(ValueError, match="vote"):
        idx.locate(fp=None, threshold=0.5, vote="histogram")
    with pytest.raises(ValueError, match="re-ranked"):
        idx.locate(fp=None, vote="diagonal", rerank=True)
    with pytest.raises(ValueError, match="vote"):
        idx.scanner(threshold=0.5, vote="histogram")
    with pytest.raises(ValueError, match="bin_rows"):
        idx.scanner(threshold=0.5, vote="diagonal", bin_rows=0)
    with pytest.raises(ValueError, match="min_hits"):
        idx.links(threshold=0.5, vote="diagonal", min_hits=0)
    with pytest.raises(ValueError, match="vote"):
        idx.links(threshold=0.5, vote="histogram")
