"""CPU: the rule of the local alignment (include/nsid.h, "locating a sample") as an oracle, its tie rules by hand, planted recovery by
the oracle alone, interval_recall, and every refusal of the ops and of SampleIndex.align / locate without a device."""
import math

import numpy as np
import pytest
import torch

from locate_oracle import (PLANT_MIN_SCORE, PLANT_NOISE, PLANT_SEEDS, PLANT_SHAPE, PLANT_THETA, PLANTS, align_cells, align_oracle,
                           align_rows, case, dyadic, occurrences, plants_matched, row_results_from_cells)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the two forms of the oracle
@pytest.mark.parametrize("Lq,Lr", [(1, 1), (2, 3), (3, 2), (33, 65), (64, 31)])
def test_row_form_equals_the_cell_loop(Lq, Lr):
    rng = np.random.default_rng(Lq * 100 + Lr)
    S = dyadic(rng, Lq, Lr)
    H, org = align_cells(S, 0.5)
    row_h, row_j, row_org, H2, org2 = align_rows(S, 0.5, want_cells=True)
    np.testing.assert_array_equal(_bits(H), _bits(H2))
    np.testing.assert_array_equal(org, org2)
    want = row_results_from_cells(S, 0.5, H, org)
    np.testing.assert_array_equal(_bits(want[0]), _bits(row_h))
    np.testing.assert_array_equal(want[1], row_j)
    np.testing.assert_array_equal(want[2], row_org)
    if Lq * Lr > 100:
        assert (H > 0).any() and (org == -1).any()
        hv = H[H > 0]
        assert hv.size > np.unique(hv).size                    # exact ties do occur


# ------------------------------------------------------------------------------------------------ by hand
def _S(Lq, Lr, cells, fill=0.0):
    S = np.full((Lq, Lr), fill, dtype=np.float32)
    for (i, j), v in cells.items():
        S[i, j] = v
    return S


def test_step_order_on_a_tie():
    # cell (2, 2) has three equal predecessors (1,1), (1,0), (0,1): the first step, (1,1), wins
    S = _S(3, 3, {(1, 1): 1.0, (1, 0): 1.0, (0, 1): 1.0, (2, 2): 1.0})
    H, org = align_cells(S, 0.5)
    assert H[1, 1] == H[1, 0] == H[0, 1] == 0.5 and H[2, 2] == 1.0
    assert org[2, 2] == (1 << 16 | 1)
    # without (1,1): (1,2) before (2,1)
    S = _S(3, 3, {(1, 0): 1.0, (0, 1): 1.0, (2, 2): 1.0})
    assert align_cells(S, 0.5)[1][2, 2] == (1 << 16 | 0)
    S = _S(3, 3, {(0, 1): 1.0, (2, 2): 1.0})
    assert align_cells(S, 0.5)[1][2, 2] == (0 << 16 | 1)
    # a strictly larger later predecessor beats an earlier one
    S = _S(3, 3, {(1, 1): 0.75, (0, 1): 1.0, (2, 2): 1.0})
    assert align_cells(S, 0.5)[1][2, 2] == (0 << 16 | 1)


def test_a_zero_predecessor_is_never_taken():
    S = _S(2, 2, {(1, 1): 1.0})                               # every predecessor of (1, 1) is zero: it starts a path of its own
    H, org = align_cells(S, 0.5)
    assert H[0, 0] == 0 and org[0, 0] == -1 and org[1, 1] == (1 << 16 | 1) and H[1, 1] == 0.5


def test_row_best_tie_goes_to_the_smaller_j():
    S = _S(1, 4, {(0, 1): 1.0, (0, 3): 1.0})
    row_h, row_j, row_org = align_rows(S, 0.5)
    assert row_h[0] == 0.5 and row_j[0] == 1 and row_org[0] == (0 << 16 | 1)


def test_a_decaying_tail_does_not_win_a_row():
    # a strong path ends at (1, 1); in row 2 its tail (2, 2) still carries H = 1.75 but does not pass the threshold itself, while a new
    # occurrence starts at (2, 0) with H = 0.25
    S = _S(3, 3, {(0, 0): 1.5, (1, 1): 1.5, (2, 2): 0.25, (2, 0): 0.75})
    H, org = align_cells(S, 0.5)
    assert H[2, 2] == 1.75 and H[2, 0] == 0.25
    row_h, row_j, row_org = align_rows(S, 0.5)
    assert row_j.tolist() == [0, 1, 0] and row_h[2] == 0.25 and row_org[2] == (2 << 16 | 0)
    # a row whose cells all fail the threshold has no result, whatever H holds
    S[2, 0] = 0.0
    row_h, row_j, row_org = align_rows(S, 0.5)
    assert (row_h[2], row_j[2], row_org[2]) == (0, -1, -1)


def test_group_tie_goes_to_the_smaller_i():
    row_h = np.array([1.0, 2.0, 2.0, 0.0], dtype=np.float32)
    row_j = np.array([3, 4, 5, -1], dtype=np.int32)
    row_org = np.array([7, 7, 7, -1], dtype=np.int32)
    occ, sc, n = occurrences(row_h, row_j, row_org, 0.0, 4)
    assert n == 1 and occ[0].tolist() == [0, 1, 7, 4] and sc[0] == 2.0
    assert occ[1].tolist() == [-1] * 4 and sc[1] == 0


def test_three_key_order_top_and_min_score():
    o = lambda i0, j0: i0 << 16 | j0
    row_h = np.array([2.0, 3.0, 2.0, 2.0, 1.0], dtype=np.float32)
    row_j = np.array([10, 11, 12, 13, 14], dtype=np.int32)
    row_org = np.array([o(2, 5), o(1, 0), o(0, 9), o(2, 1), o(0, 0)], dtype=np.int32)
    occ, sc, n = occurrences(row_h, row_j, row_org, 0.0, 8)
    assert n == 5
    # score descending, then i0 ascending, then j0 ascending
    assert occ[:5].tolist() == [[1, 1, 0, 11], [0, 2, 9, 12], [2, 3, 1, 13], [2, 0, 5, 10], [0, 4, 0, 14]]
    assert sc[:5].tolist() == [3.0, 2.0, 2.0, 2.0, 1.0] and occ[5:].max() == -1 and sc[5:].max() == 0
    occ, sc, n = occurrences(row_h, row_j, row_org, 0.0, 2)      # n_occ > top: the count is of the kept, the slots the first top
    assert n == 5 and occ.tolist() == [[1, 1, 0, 11], [0, 2, 9, 12]]
    occ, sc, n = occurrences(row_h, row_j, row_org, 2.0, 8)      # min_score exactly met is kept (>=)
    assert n == 4 and sc[:4].tolist() == [3.0, 2.0, 2.0, 2.0]
    occ, sc, n = occurrences(row_h, row_j, row_org, np.nextafter(np.float32(2.0), np.float32(3.0)), 8)
    assert n == 1


def test_a_loop_gives_one_occurrence_per_repetition():
    # the same three song rows twice in the query, nothing in between: the second repetition starts at a cell whose predecessors are zero
    S = _S(8, 3, {(0, 0): 1.0, (1, 1): 1.0, (2, 2): 1.0, (4, 0): 1.0, (5, 1): 1.0, (6, 2): 1.0})
    occ, sc, n, *_ = align_oracle(S, 0.5, 1.0, 4)
    assert n == 2 and occ[:2].tolist() == [[0, 2, 0, 2], [4, 6, 0, 2]] and sc[:2].tolist() == [1.5, 1.5]


@pytest.mark.parametrize("seed", list(PLANT_SEEDS))
def test_planted_occurrences_are_recovered_by_the_oracle(seed):
    """the condition under which the GPU test is allowed its +-1 row"""
    q, ref = case(seed, *PLANT_SHAPE, PLANTS, PLANT_NOISE)
    S = (q.astype(np.float64) @ ref.astype(np.float64).T).astype(np.float32)
    occ, sc, n, *_ = align_oracle(S, PLANT_THETA, PLANT_MIN_SCORE, 16)
    assert plants_matched(occ, n), (n, occ[:max(n, 0)].tolist())
    assert (sc[:n] >= PLANT_MIN_SCORE).all() and (np.diff(sc[:n]) <= 0).all()


# ------------------------------------------------------------------------------------------------ interval_recall
def test_interval_recall_by_hand():
    from neuralsampleid_amd.identify import interval_recall
    # partial cover on both sides of min_cover: 4.9 of 10 s is not found, 5.0 of 10 s is
    r, cov, out = interval_recall([(0.0, 4.9)], [(0.0, 10.0)])
    assert r == 0.0 and cov == pytest.approx(4.9) and out == pytest.approx(0.0)
    r, cov, out = interval_recall([(-2.0, 5.0)], [(0.0, 10.0)])
    assert r == 1.0 and cov == pytest.approx(5.0) and out == pytest.approx(2.0)
    assert interval_recall([(0.0, 3.0)], [(0.0, 10.0)], min_cover=0.3)[0] == 1.0
    # overlapping found intervals count once: their union covers 6 of 10 s
    r, cov, out = interval_recall([(0.0, 4.0), (2.0, 6.0), (20.0, 21.0)], [(0.0, 10.0), (30.0, 40.0)])
    assert r == 0.5 and cov == pytest.approx(6.0) and out == pytest.approx(1.0)
    # two found pieces that only together reach the cover
    assert interval_recall([(0.0, 3.0), (7.0, 10.0)], [(0.0, 10.0)])[0] == 1.0
    # empty lists
    r, cov, out = interval_recall([], [(0.0, 1.0)])
    assert (r, cov, out) == (0.0, 0.0, 0.0)
    r, cov, out = interval_recall([(1.0, 3.0)], [])
    assert math.isnan(r) and cov == 0.0 and out == pytest.approx(2.0)
    assert math.isnan(interval_recall([], [])[0])
    with pytest.raises(ValueError):
        interval_recall([(2.0, 1.0)], [(0.0, 1.0)])


# ------------------------------------------------------------------------------------------------ names, limits, refusals
def test_names_and_limits():
    from neuralsampleid_amd import _lib, ops
    assert "nsid_pair_sim" in _lib.SIGNATURES and "nsid_local_align" in _lib.SIGNATURES
    assert (ops.ALIGN_MAX_ROWS, ops.ALIGN_MAX_COLS, ops.ALIGN_MAX_TOP) == (4096, 4096, 64)
    assert (ops.ALIGN_MAX_ROWS, ops.ALIGN_MAX_COLS, ops.ALIGN_MAX_TOP) == tuple(
        _lib.DEFINES[k] for k in ("NSID_ALIGN_MAX_ROWS", "NSID_ALIGN_MAX_COLS", "NSID_ALIGN_MAX_TOP"))
    c = ops.launch_counters()
    assert "pair_sim" in c and "local_align" in c


def test_pair_sim_tiles_cover_every_pair_largest_first():
    from neuralsampleid_amd import ops
    q_len, x_len = [33, 0, 64, 1, 5], [65, 7, 31, 1, 0]
    t = ops.pair_sim_tiles(q_len, x_len)
    assert t.dtype == np.int32 and t.shape == (6 + 2 + 1, 3)
    assert t[:, 0].tolist() == [0] * 6 + [2] * 2 + [3]
    for p in (0, 2, 3):
        cover = np.zeros((q_len[p], x_len[p]), dtype=int)
        for _, i0, j0 in t[t[:, 0] == p].tolist():
            cover[i0:i0 + 32, j0:j0 + 32] += 1
        assert (cover == 1).all()
    assert ops.pair_sim_tiles([], []).shape == (0, 3)


def test_ops_refuse_before_any_launch():
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    q, x = torch.zeros(8, 128), torch.zeros(9, 128)
    with pytest.raises(RuntimeError):
        ops.pair_sim(q, x, [0], [8], [0], [9])                                   # CPU tensors
    with pytest.raises(RuntimeError):
        ops.local_align(torch.zeros(72), [0], [9], [8], [9], 0.5)
    with pytest.raises(TypeError):
        ops.local_align(np.zeros(72, np.float32), [0], [9], [8], [9], 0.5)
    with pytest.raises(RuntimeError):
        ops.pair_sim(q.double(), x.double(), [0], [8], [0], [9])                 # dtype
    with pytest.raises(RuntimeError):
        ops.pair_sim(q[0], x, [0], [8], [0], [9])                                # rank
    # sizes past the limits are refused ahead of the tensors, so they show without a device
    big = torch.zeros(4097, 128)
    with pytest.raises(ValueError, match="4096"):
        ops.pair_sim(big, x, [0], [4097], [0], [9])
    with pytest.raises(ValueError, match="4096"):
        ops.pair_sim(q, big, [0], [8], [0], [4097])
    with pytest.raises(ValueError):
        ops.pair_sim(q, x, [0], [8], [0], [-1])
    with pytest.raises(ValueError):
        ops.pair_sim(q, x, [0], [8, 8], [0], [9])                                # one entry per pair
    # local_align looks at its tensor first (a CPU tensor is a RuntimeError whatever the sizes); its limits are the C entry's, which
    # checks them before it launches or reads anything: null pointers stand for the tensors
    from neuralsampleid_amd._lib import DEFINES, lib
    einval = DEFINES["NSID_EINVAL"]

    def c_align(npairs=1, max_q=8, max_x=9, theta=0.5, min_score=0.0, top=16):
        return lib.nsid_local_align(None, None, None, None, None, npairs, max_q, max_x, theta, min_score, top, None, None, None, None,
                                    None, None, None, None)
    assert c_align(npairs=0) == 0                                                # nothing to do
    assert c_align() == einval                                                   # null tables
    for kw in ({"max_q": 4097}, {"max_x": 4097}, {"top": 0}, {"top": 65}, {"npairs": -1}, {"max_q": -1}, {"theta": float("nan")},
               {"min_score": float("nan")}):
        assert c_align(**{"npairs": 0, **kw}) == einval, kw                      # refused although there is no pair to run
    for d in (0, 8, 100, 264, 2112):
        assert lib.nsid_pair_sim(None, d, 0, None, d, 0, d, None, None, None, None, None, None, 0, None, 0, None, 0, None) == einval
    assert lib.nsid_pair_sim(None, 128, 0, None, 128, 0, 128, None, None, None, None, None, None, 0, None, 0, None, 0, None) == 0
    assert ops.launch_counters() == before


def test_sample_index_refuses_before_the_device():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    before = ops.launch_counters()
    idx = SampleIndex(None)
    fp = torch.zeros(10, 128)
    with pytest.raises(ValueError, match="threshold"):
        idx.align(fp, [])                                                        # no threshold without rerank
    with pytest.raises(ValueError, match="threshold"):
        idx.locate(fp=fp)
    with pytest.raises(RuntimeError, match="classifier"):
        idx.align(fp, [], rerank=True)                                           # rerank without a classifier
    with pytest.raises(RuntimeError, match="classifier"):
        idx.locate(fp=fp, rerank=True)
    with pytest.raises(KeyError):
        idx.align(fp, ["no such song"], threshold=0.5)                           # unknown song name
    with pytest.raises(KeyError):
        idx.locate(fp=fp, threshold=0.5, exclude="no such song")
    with pytest.raises(ValueError):
        idx.align(fp[0], [], threshold=0.5)                                      # rank
    with pytest.raises(ValueError):
        idx.align(fp.double(), [], threshold=0.5)                                # dtype
    with pytest.raises(TypeError):
        idx.align(fp.numpy(), [], threshold=0.5)
    with pytest.raises(ValueError):
        idx.align(torch.zeros(10, 100), [], threshold=0.5)                       # d outside the search's widths
    with pytest.raises(ValueError, match="4096"):
        idx.align(torch.zeros(4097, 128), [], threshold=0.5)                     # past the limit
    with pytest.raises(ValueError, match="4096"):
        idx.locate(fp=torch.zeros(4097, 128), threshold=0.5)
    for top in (0, 65):
        with pytest.raises(ValueError, match="top"):
            idx.align(fp, [], threshold=0.5, top=top)
    with pytest.raises(ValueError):
        idx.align(fp, [], threshold=float("nan"))
    with pytest.raises(ValueError):
        idx.align(fp, [], threshold=0.5, row_hop_s=0.5)                          # half a row timing
    with pytest.raises(TypeError):
        idx.align(fp, "abc", threshold=0.5)
    with pytest.raises(ValueError):
        idx.locate(fp=fp, threshold=0.5, n_songs=0)
    with pytest.raises(ValueError):
        idx.locate(fp=fp, threshold=0.5, k_probe=65)
    with pytest.raises(RuntimeError):
        idx.align(fp, [], threshold=0.5)                                         # a CPU tensor, everything else in order
    with pytest.raises(RuntimeError):
        idx.locate(fp=fp, threshold=0.5)
    assert ops.launch_counters() == before
