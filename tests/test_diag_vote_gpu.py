"""GPU: ops.diag_vote against the oracle of the rule (diag_vote_oracle.py), every output array equal exactly. I is synthesized, so no
database is needed."""
import numpy as np
import pytest
import torch

from diag_vote_oracle import diag_vote as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("songs", "counts", "i_lo", "i_hi", "r_lo", "r_hi", "n_songs")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(I, starts, lens, song_of, n_dummy, exclude, bin_rows, top, msg=""):
    from neuralsampleid_amd import ops
    before = ops.launch_counters()["diag_vote"]
    got = ops.diag_vote(_dev(I), starts, lens, _dev(np.asarray(song_of, dtype=np.int32)), n_dummy, exclude, bin_rows, top)
    assert ops.launch_counters()["diag_vote"] == before + (1 if len(starts) else 0)          # one launch for all pairs
    want = oracle(I, starts, lens, song_of, n_dummy, exclude, bin_rows, top)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == torch.int32 and g.is_cuda
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{msg} {name}")
    return want


def _table(rng, rows, k, n_ref, n_songs, n_dummy, diagonals=4, dead=0.05):
    """a search result with everything the vote skips in it, some diagonals and repeated candidates; song_of in blocks (sorted codes)
    with rows that never vote"""
    cuts = np.sort(rng.choice(np.arange(1, n_ref), size=min(n_songs, n_ref) - 1, replace=False)) if n_songs > 1 else np.zeros(0, int)
    song_of = np.searchsorted(cuts, np.arange(n_ref), side="right").astype(np.int32)
    song_of[rng.random(n_ref) < dead] = -1
    I = rng.integers(0, n_dummy + n_ref + 3, size=(rows, k)).astype(np.int64)          # dummy ids, ref ids, 3 ids past the end
    for _ in range(diagonals):                                                         # r = r0 + rate * row, one column
        r0, rate, col = int(rng.integers(0, n_ref)), float(rng.choice([0.8, 1.0, 1.25])), int(rng.integers(0, k))
        a = int(rng.integers(0, rows))
        b = int(rng.integers(a, rows)) + 1
        r = r0 + np.round(rate * np.arange(b - a)).astype(np.int64)
        ok = r < n_ref
        I[a:b, col][ok] = n_dummy + r[ok]
    if k > 1:
        rep = rng.random(rows) < 0.1
        I[rep, 1] = I[rep, 0]                                                          # a repeated candidate
        tail = rng.random(rows) < 0.1
        I[tail, k - 1] = -1                                                            # the -1 tail of a short search result
    return I, song_of


# (L, k) of the longest pair, bin_rows, top, songs, n_ref. L k = 4096 three ways, 4080, L = 1, k = 1; more and fewer songs than top
SHAPES = [(64, 64, 16, 10, 40, 700), (4096, 1, 16, 32, 300, 5000), (2048, 2, 1, 1, 300, 5000), (204, 20, 16, 10, 40, 2560),
          (204, 20, 4096, 32, 5, 500), (204, 20, 1, 32, 100, 900), (1, 20, 16, 1, 3, 50), (50, 1, 16, 32, 200, 400), (7, 3, 2, 10, 4, 30)]


@pytest.mark.parametrize("L, k, bin_rows, top, n_songs, n_ref", SHAPES)
def test_diag_vote_matches_oracle(L, k, bin_rows, top, n_songs, n_ref):
    rng = np.random.default_rng(L * 131 + k)
    n_dummy = 17
    rows = L + 9
    I, song_of = _table(rng, rows, k, n_ref, n_songs, n_dummy)
    # the longest pair at two starts, pairs that share rows, one row, the last row
    starts = [0, 9, 3, 3, rows - 1, 0]
    lens = [L, L, max(1, L // 2), max(1, L // 3), 1, 1]
    exclude = [-1, int(song_of[song_of >= 0][0]), -1, n_songs - 1, -1, 0]
    want = _check(I, starts, lens, song_of, n_dummy, exclude, bin_rows, top, "exclude")
    _check(I, starts, lens, song_of, n_dummy, None, bin_rows, top, "no exclude")
    assert (want[6] >= 0).all() and want[6][0] >= 1
    if n_songs > 2 * top and L * k >= 2000:
        assert want[6][0] > top                                        # more songs than top
    if n_songs < top:
        assert (want[0][0] == -1).any()                                # fewer


def test_one_key_distinct_keys_and_ties():
    # all 4096 hits on one key: one song, bin_rows = 4096 and delta < 4096
    rng = np.random.default_rng(5)
    I = rng.integers(0, 100, size=(64, 64)).astype(np.int64)
    want = _check(I, [0], [64], [3] * 100, 0, None, 4096, 10, "one key")
    assert want[1][0, 0] == 4096 and want[6][0] == 1 and want[2][0, 0] == 0 and want[3][0, 0] == 63
    # 4096 distinct keys in one song: r = 2 i -> delta = i + 4095, bin_rows = 1; every wide bin holds two hits, the first one wins
    I = (2 * np.arange(4096, dtype=np.int64)).reshape(4096, 1)
    want = _check(I, [0], [4096], [0] * 8192, 0, None, 1, 10, "distinct keys, one song")
    assert want[1][0, 0] == 2 and (want[2][0, 0], want[3][0, 0]) == (0, 1)
    # 4096 distinct songs: every song one hit, ranked by code
    song_of = np.arange(8192, dtype=np.int32)
    want = _check(I, [0], [4096], song_of, 0, None, 16, 32, "distinct songs")
    assert want[0][0].tolist() == list(range(0, 64, 2)) and want[6][0] == 4096
    # the hand-made ties of test_diag_vote_cpu.py: two songs with equal scores, two bins with equal counts
    want = _check(np.asarray([[8, 0], [9, 1]], dtype=np.int64), [0], [2], [0] * 8 + [1] * 8, 0, None, 4, 3, "two songs tie")
    assert want[0][0].tolist() == [0, 1, -1] and want[1][0].tolist() == [2, 2, 0]
    want = _check(np.asarray([[20, 0], [21, 1]], dtype=np.int64), [0], [2], [0] * 32, 0, None, 4, 3, "two bins tie")
    assert (want[4][0, 0], want[5][0, 0]) == (0, 1)
    want = _check(np.asarray([[3, 16], [5, 17], [7, 18], [9, -1]], dtype=np.int64), [0], [4], [0] * 16 + [1] * 16, 0, None, 4, 3, "edge")
    assert want[1][0].tolist() == [4, 3, 0]


def test_ids_at_the_top_of_the_int32_range():
    rng = np.random.default_rng(9)
    n_ref = 600
    n_dummy = 2 ** 31 - 1 - n_ref
    I, song_of = _table(rng, 110, 20, n_ref, 12, 0)
    I = np.where(I >= 0, I + n_dummy, I)                               # the 3 ids past the end are past 2^31 - 1
    I[5, 0], I[6, 0] = n_dummy - 1, 7                                  # dummy ids
    want = _check(I, [0, 10], [100, 100], song_of, n_dummy, [-1, 2], 16, 10, "large ids")
    assert want[5].max() < n_ref and want[6].min() > 1


def test_a_bad_pair_beside_valid_ones_and_no_pairs():
    """the lengths live on the device: ops refuses a pair past 4096 candidates, the kernel itself gives it an empty row and leaves its
    neighbours alone (the entry called as ops calls it)"""
    from neuralsampleid_amd import _lib, ops
    rng = np.random.default_rng(3)
    I, song_of = _table(rng, 300, 20, 900, 30, 5)
    starts, lens = [0, 0, 50, 0], [204, 205, 100, 0]                  # 205 x 20 = 4100 candidates; a pair of no rows
    Id, so = _dev(I), _dev(song_of)
    st, ln = _dev(np.asarray(starts, dtype=np.int32)), _dev(np.asarray(lens, dtype=np.int32))
    top = 10
    out = [torch.full((4, top), -777, device=DEV, dtype=torch.int32) for _ in range(6)] + [torch.full((4,), -777, device=DEV,
                                                                                                        dtype=torch.int32)]
    _lib.call("nsid_diag_vote", Id.data_ptr(), 20, st.data_ptr(), ln.data_ptr(), 4, so.data_ptr(), 900, 5, None, 16, top,
              *(t.data_ptr() for t in out), torch.cuda.current_stream().cuda_stream)
    want = oracle(I, starts, lens, song_of, 5, None, 16, top)
    assert want[6].tolist()[1] == -1 and want[6].tolist()[3] == -1 and want[6][0] > 0 and want[6][2] > 0
    for name, g, w in zip(NAMES, out, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    with pytest.raises(ValueError, match="4096"):
        ops.diag_vote(Id, starts[:2], lens[:2], so, 5)
    # no pairs: empty results, nothing launched
    before = ops.launch_counters()["diag_vote"]
    got = ops.diag_vote(Id, [], [], so, 5, None, 16, 7)
    assert [tuple(t.shape) for t in got] == [(0, 7)] * 6 + [(0,)] and ops.launch_counters()["diag_vote"] == before


def test_refusals_come_before_any_launch():
    from neuralsampleid_amd import ops
    I = torch.zeros((10, 20), device=DEV, dtype=torch.int64)
    so = torch.zeros(8, device=DEV, dtype=torch.int32)
    before = ops.launch_counters()
    for fn in (lambda: ops.diag_vote(I, [0], [10], so, 0, None, 0), lambda: ops.diag_vote(I, [0], [10], so, 0, None, 4097),
               lambda: ops.diag_vote(I, [0], [10], so, 0, None, 16, 0), lambda: ops.diag_vote(I, [0], [10], so, 0, None, 16, 33),
               lambda: ops.diag_vote(I, [0], [11], so, 0), lambda: ops.diag_vote(I, [0], [0], so, 0),
               lambda: ops.diag_vote(I, [0, 1], [1], so, 0), lambda: ops.diag_vote(I, [0], [10], so, 0, [1, 2]),
               lambda: ops.diag_vote(I, [0], [10], so, -1), lambda: ops.diag_vote(I, [0], [10], so, 2 ** 31 - 8),
               lambda: ops.diag_vote(torch.zeros((4, 65), device=DEV, dtype=torch.int64), [0], [1], so, 0)):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: ops.diag_vote(I.cpu(), [0], [10], so, 0), lambda: ops.diag_vote(I.int(), [0], [10], so, 0),
               lambda: ops.diag_vote(I, [0], [10], so.long(), 0), lambda: ops.diag_vote(I.t(), [0], [10], so, 0)):
        with pytest.raises(RuntimeError):
            fn()
    assert ops.launch_counters() == before
