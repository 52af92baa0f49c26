"""CPU: the fact that alignment paths rest on (the rule on an occurrence's box alone gives the path of the whole matrix, bit for bit), the
two forms of the path oracle, AlignmentPath's derived fields by hand, the fitted line on the planted cases, and the binding."""
import math

import numpy as np
import pytest

from align_path_oracle import NONE, band, box_path, cells_from, line, rows_from, trace
from locate_oracle import (PLANT_MIN_SCORE, PLANT_NOISE, PLANT_SEEDS, PLANT_SHAPE, PLANT_THETA, PLANTS, STEPS, align_cells, align_oracle,
                           case, dyadic)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the two forms of the oracle
@pytest.mark.parametrize("Lq,Lr", [(1, 1), (2, 3), (3, 2), (33, 65), (64, 31)])
def test_row_form_equals_the_cell_loop(Lq, Lr):
    rng = np.random.default_rng(Lq * 100 + Lr)
    S = dyadic(rng, Lq, Lr)
    for theta in (0.25, 0.5):
        H, frm = cells_from(S, theta)
        H2, frm2 = rows_from(S, theta)
        np.testing.assert_array_equal(_bits(H), _bits(H2))
        np.testing.assert_array_equal(frm, frm2)
        np.testing.assert_array_equal(_bits(H), _bits(align_cells(S, theta)[0]))       # and the H of the oracle that keeps origins
        assert ((frm == NONE) | (H > 0)).all()
    if Lq * Lr > 100:
        assert sorted(np.unique(frm).tolist()) == [0, 1, 2, 3]                      # every step is taken somewhere


def test_band_matrices_hold_one_long_path():
    rng = np.random.default_rng(3)
    for rate, shape in ((0.5, (120, 60)), (1.0, (80, 80)), (2.0, (60, 120))):
        S = band(rng, *shape, rate)
        assert (S != 0).sum() <= 7 * shape[0] and set(np.unique(S).tolist()) <= {0.0, 0.25, -0.25, 0.375, 0.5, 0.625, 0.75, 1.0}
        H, frm = rows_from(S, 0.375)
        i, j = np.unravel_index(np.argmax(H), H.shape)
        pi, pj = trace(frm, int(i), int(j))
        assert pi.size >= min(shape) // 3                                           # a path over a good part of the band


# ------------------------------------------------------------------------------------------------ the box against the whole matrix
def test_the_box_alone_gives_the_path_of_the_whole_matrix():
    """On tie-heavy matrices: for every occurrence, the rule on its box alone traces cell for cell the path of the whole matrix, from the
    box's first cell, and the last H has the score's bits."""
    rng = np.random.default_rng(11)
    n_mats = n_occs = long_paths = steps_seen = 0
    for n in range(102):
        Lq, Lr = (int(v) for v in rng.integers(1, 49, size=2))
        if n < 4:
            Lq, Lr = ((48, 48), (47, 40), (1, 1), (2, 3))[n]
        S = dyadic(rng, Lq, Lr)
        for theta in (0.25, 0.375, 0.5):
            n_mats += 1
            H, frm = cells_from(S, theta)
            occ, sc, n_occ = align_oracle(S, theta, 0.0, 64)[:3]
            for (i0, i1, j0, j1), score in zip(occ[:min(n_occ, 64)].tolist(), sc.tolist()):
                n_occs += 1
                fi, fj = trace(frm, i1, j1)                                         # the whole matrix
                assert (fi[0], fj[0]) == (i0, j0) and _bits(H[i1, j1]) == _bits(score)
                bi, bj, end_h = box_path(S, theta, i0, i1, j0, j1, form=cells_from)
                assert bi is not None, (S.shape, theta, (i0, i1, j0, j1))
                np.testing.assert_array_equal(bi, fi)
                np.testing.assert_array_equal(bj, fj)
                assert (bi[0], bj[0]) == (i0, j0) and _bits(end_h) == _bits(score)
                ri, rj, rend = box_path(S, theta, i0, i1, j0, j1)                   # the row form on the box
                assert np.array_equal(ri, fi) and np.array_equal(rj, fj) and _bits(rend) == _bits(score)
                long_paths += fi.size >= 8
                steps_seen |= sum(1 << (3 * int(a) + int(b)) for a, b in set(zip(np.diff(fi).tolist(), np.diff(fj).tolist())))
    assert n_mats == 306 and n_occs >= 900 and long_paths >= 20
    assert steps_seen == sum(1 << (3 * a + b) for a, b in STEPS)                    # all three steps, and nothing else


def test_a_box_that_is_no_occurrence_is_told_apart():
    S = np.zeros((4, 4), np.float32)
    for t in range(1, 4):
        S[t, t] = 1.0
    # the path (1,1) (2,2) (3,3): its own box traces it; a box that starts a row and a column early does not end at its first cell
    pi, pj, h = box_path(S, 0.5, 1, 3, 1, 3)
    assert pi.tolist() == [1, 2, 3] and pj.tolist() == [1, 2, 3] and h == np.float32(1.5)
    assert box_path(S, 0.5, 0, 3, 0, 3)[0] is None and box_path(S, 0.5, 0, 3, 0, 3)[2] == np.float32(1.5)
    assert box_path(S, 0.5, 1, 3, 1, 2)[0] is None and box_path(S, 0.5, 1, 3, 1, 2)[2] == 0            # the last H is not positive


# ------------------------------------------------------------------------------------------------ AlignmentPath by hand
def _occ(i0, i1, j0, j1, score=1.0):
    from neuralsampleid_amd.identify import _occurrence
    return _occurrence("song", score, i0, i1, j0, j1, None)


def test_alignment_path_fields_by_hand():
    from neuralsampleid_amd.identify import AlignmentPath, alignment_path
    q, r = [10, 11, 12, 14, 15], [20, 21, 23, 24, 25]                               # (1,1) (1,2) (2,1) (1,1)
    s = np.asarray([0.75, 0.5, 0.625, 0.25, 1.0], np.float32)
    p = alignment_path(_occ(10, 15, 20, 25), q, r, s, 0.5, timing=(0.5, 1.0))
    assert isinstance(p, AlignmentPath) and p.occurrence.q_rows == (10, 15)
    assert p.q_rows.dtype == np.int32 and p.r_rows.dtype == np.int32 and p.scores.dtype == np.float32
    assert p.steps == (2, 1, 1) and sum(p.steps) == len(q) - 1
    assert p.passing == 3                                                           # 0.5 - 0.5 is not positive, 0.25 is below
    a, b = np.polyfit(np.asarray(q, float), np.asarray(r, float), 1)
    assert math.isclose(p.slope, a, rel_tol=1e-12) and math.isclose(p.intercept, b, rel_tol=1e-12)
    res = np.asarray(r, float) - (a * np.asarray(q, float) + b)
    assert math.isclose(p.rms_rows, float(np.sqrt((res ** 2).mean())), rel_tol=1e-9)
    # song_row: at the cells, between them (the (2,1) step passes query row 13 half way), and clamped outside
    assert [float(p.song_row(v)) for v in q] == [float(v) for v in r]
    assert float(p.song_row(13)) == 23.5 and float(p.song_row(11.5)) == 22.0
    assert float(p.song_row(0)) == 20.0 and float(p.song_row(99)) == 25.0
    np.testing.assert_array_equal(p.song_row(np.asarray([10, 13, 40])), [20.0, 23.5, 25.0])
    np.testing.assert_array_equal(p.q_time, np.asarray(q) * 0.5)
    np.testing.assert_array_equal(p.r_time, np.asarray(r) * 0.5)
    assert float(p.song_time(6.5)) == 11.75 and float(p.song_time(0.0)) == 10.0 and float(p.song_time(1e9)) == 12.5


def test_alignment_path_of_a_straight_line_one_cell_and_no_timing():
    from neuralsampleid_amd.identify import alignment_path
    p = alignment_path(_occ(0, 9, 5, 14), np.arange(10), np.arange(10) + 5, np.ones(10, np.float32), 0.25)
    assert p.steps == (9, 0, 0) and p.passing == 10 and p.slope == 1.0 and p.intercept == 5.0 and p.rms_rows == 0.0
    assert p.q_time is None and p.r_time is None
    with pytest.raises(ValueError, match="timing"):
        p.song_time(1.0)
    one = alignment_path(_occ(3, 3, 4, 4), [3], [4], [0.75], 0.5)
    assert one.steps == (0, 0, 0) and one.passing == 1 and one.slope is None and one.intercept is None and one.rms_rows is None
    assert float(one.song_row(0)) == 4.0 and float(one.song_row(3)) == 4.0
    # passing is an fp32 compare: a threshold that only fp64 tells from the score passes nothing
    assert alignment_path(_occ(3, 3, 4, 4), [3], [4], [np.float32(0.1)], 0.1).passing == 0
    for bad in (([1, 2], [1, 4]), ([1, 1], [1, 2]), ([1, 3], [1, 3]), ([2, 1], [2, 1])):      # not steps of the rule
        with pytest.raises(ValueError, match="follow"):
            alignment_path(_occ(1, 2, 1, 2), bad[0], bad[1], [1.0, 1.0], 0.5)
    with pytest.raises(ValueError):
        alignment_path(_occ(1, 2, 1, 2), [], [], [], 0.5)


# ------------------------------------------------------------------------------------------------ the planted cases
def test_the_fitted_line_is_the_better_tempo_estimate_on_the_planted_cases():
    """through the oracle: the line's slope is within 0.1 of every planted rate and never further from it than the end-point ratio"""
    from neuralsampleid_amd.identify import alignment_path
    Lq, Lr, d = PLANT_SHAPE
    worst, n = 0.0, 0
    for seed in PLANT_SEEDS:
        q, ref = case(seed, Lq, Lr, d, PLANTS, PLANT_NOISE)
        S = (q.astype(np.float64) @ ref.astype(np.float64).T).astype(np.float32)
        occ, sc, n_occ = align_oracle(S, PLANT_THETA, PLANT_MIN_SCORE, 16)[:3]
        assert n_occ == len(PLANTS)
        for a, b, rows, rate in PLANTS:
            hits = [(o, s) for o, s in zip(occ[:n_occ].tolist(), sc.tolist()) if abs(o[0] - a) <= 1 and abs(o[2] - b) <= 1]
            assert len(hits) == 1
            (i0, i1, j0, j1), score = hits[0]
            pi, pj, end_h = box_path(S, PLANT_THETA, i0, i1, j0, j1)
            assert pi is not None and _bits(end_h) == _bits(score)
            p = alignment_path(_occ(i0, i1, j0, j1, score), pi, pj, S[pi, pj], PLANT_THETA)
            assert math.isclose(p.slope, line(pi, pj)[0], rel_tol=1e-9)
            stretch = (j1 - j0) / (i1 - i0)
            print(f"seed {seed} plant rate {rate}: slope {p.slope:.4f} stretch {stretch:.4f} rms {p.rms_rows:.3f} steps {p.steps} "
                  f"passing {p.passing}/{pi.size}")
            assert abs(p.slope - rate) <= 0.1, (seed, rate, p.slope)
            assert abs(p.slope - rate) <= abs(stretch - rate), (seed, rate, p.slope, stretch)
            worst = max(worst, abs(p.slope - rate))
            n += 1
    assert n == 24 and worst > 0.0


# ------------------------------------------------------------------------------------------------ the binding
def test_the_header_names_the_entry_and_the_limit():
    from neuralsampleid_amd import _lib, ops
    assert _lib.PROTOTYPES["nsid_align_paths"] == ("i", "ppppppp" + "iif" + "pp" + "pppppp" + "s")
    assert "nsid_align_paths" in _lib.EXPORTS and hasattr(_lib.lib, "nsid_align_paths")
    assert _lib.DEFINES["NSID_ALIGN_PATH_MAX"] == 4096 == ops.ALIGN_PATH_MAX
    assert "align_paths" in ops.launch_counters()
    ws = _lib.lib.nsid_workspace_bytes
    assert [ws(b"align_paths", r, c) for r, c in ((1, 1), (3, 4), (3, 5), (0, 9), (9, 0), (4096, 4096))] == [1, 3, 6, 0, 0, 4096 * 1024]


def test_the_entry_checks_its_arguments_without_a_device():
    """zero boxes: NSID_OK with nothing launched, whatever the pointers; NaN theta and a bound past the limit: NSID_EINVAL"""
    from neuralsampleid_amd import _lib
    lib, N = _lib.lib, None
    _lib.launch_counters(reset=True)
    args = lambda nb, max_cols, theta: (N, N, N, N, N, N, N, nb, max_cols, theta, N, N, N, N, N, N, N, N, N)
    assert lib.nsid_align_paths(*args(0, 4096, 0.5)) == 0
    assert lib.nsid_align_paths(*args(0, 4097, 0.5)) == -1
    assert lib.nsid_align_paths(*args(0, -1, 0.5)) == -1
    assert lib.nsid_align_paths(*args(-1, 16, 0.5)) == -1
    assert lib.nsid_align_paths(*args(0, 16, float("nan"))) == -1
    assert lib.nsid_align_paths(*args(3, 16, 0.5)) == -1                            # null pointers with boxes to do
    assert sum(_lib.launch_counters().values()) == 0


def test_paths_refuses_without_a_device():
    import torch
    from neuralsampleid_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.align_paths(torch.zeros(16), [0], [4], [4], [4], 0.5)
    with pytest.raises(TypeError):
        ops.align_paths(np.zeros(16, np.float32), [0], [4], [4], [4], 0.5)
