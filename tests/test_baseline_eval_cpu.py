"""CPU: the host side of neuralsampleid_amd/baseline_eval.py: the baseline's song vote on the reference-made golden
(tests/golden/make_baseline_eval_golden.py) and on hand-made I / D, and the argument checks that come before any GPU work."""
import json

import numpy as np
import pytest

N_DUMMY = 10
REF = ["a", "a", "b", "b", "c", "q0"]           # ids 10 .. 15


def _ID(rows):
    """rows of (id, distance) pairs -> (I int64, D float32), padded with (-1, inf)"""
    k = max(len(r) for r in rows)
    I = np.full((len(rows), k), -1, np.int64)
    D = np.full((len(rows), k), np.inf, np.float32)
    for i, r in enumerate(rows):
        for j, (c, d) in enumerate(r):
            I[i, j], D[i, j] = c, d
    return I, D


@pytest.fixture(scope="module")
def golden():
    from make_baseline_eval_golden import load_golden_inputs, standin_search
    z, inp = load_golden_inputs()
    p = json.loads(bytes(z["params"]).decode())
    D, I = standin_search(inp, p)
    np.testing.assert_array_equal(I, z["I"].astype(np.int64))
    return z, inp, p, I, D


def test_hit_rates_from_the_golden(golden):
    from neuralsampleid_amd.baseline_eval import hit_rates_baseline
    z, inp, p, I, D = golden
    assert D.dtype == np.float32
    hr, raw, ids = hit_rates_baseline(I, D, inp["query_lookup"], inp["ref_lookup"], p["n_dummy"], inp["gt"], p["test_seq_len"])
    for got, name in ((hr, "hit_rates"), (raw, "raw_score"), (ids, "test_ids")):
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])


def test_map_from_the_golden(golden):
    from neuralsampleid_amd.baseline_eval import predictions_baseline
    from neuralsampleid_amd.rerank import calculate_map
    z, inp, p, I, D = golden
    pred = predictions_baseline(I, D, inp["query_lookup"], inp["ref_lookup"], p["n_dummy"])
    want = json.loads(str(z["predictions"]))
    assert pred == want and list(pred) == list(want)
    assert abs(calculate_map(inp["gt"], pred, k=p["k_map"]) - float(z["map_score"])) <= 1e-12


def test_vote_skips_dummy_none_and_own_song():
    from neuralsampleid_amd.baseline_eval import vote_baseline
    I, D = _ID([[(3, 9.0), (10, 1.0), (15, 5.0)], [(12, 2.0), (-1, np.inf)]])
    assert vote_baseline(I, D, slice(0, 2), "q0", REF, N_DUMMY) == ["b", "a"]
    # the rows of the slice only
    assert vote_baseline(I, D, slice(0, 1), "q0", REF, N_DUMMY) == ["a"]
    assert vote_baseline(I, D, [1], "q0", REF, N_DUMMY) == ["b"]
    assert vote_baseline(I, D, slice(0, 2), "a", REF, N_DUMMY) == ["q0", "b"]
    assert vote_baseline(*_ID([[(3, 1.0), (-1, np.inf)]]), slice(0, 1), "q0", REF, N_DUMMY) == []


def test_vote_takes_the_max_of_a_repeated_candidate_and_ranks_descending():
    from neuralsampleid_amd.baseline_eval import vote_baseline
    # id 10 (a) met in both rows: max(1, 4) = 4, not 5; a = 4 + 0.5 (id 11), b = 4.25, c = 6
    I, D = _ID([[(10, 1.0), (12, 4.25), (14, 6.0)], [(10, 4.0), (11, 0.5)]])
    assert vote_baseline(I, D, slice(0, 2), "q0", REF, N_DUMMY) == ["c", "a", "b"]
    # were the two distances of id 10 added, a = 5.5 would still be second; were the minimum taken, a = 1.5 would be last
    I, D = _ID([[(10, 1.0), (12, 3.0)], [(10, 4.0)]])
    assert vote_baseline(I, D, slice(0, 2), "q0", REF, N_DUMMY) == ["a", "b"]


def test_vote_ties_keep_first_appearance_in_ascending_id_order():
    from neuralsampleid_amd.baseline_eval import vote_baseline
    # c (id 14) comes first in the row, but the walk is by ascending id: a (10), b (12), c (14) all at 2.0
    I, D = _ID([[(14, 2.0), (12, 2.0), (10, 2.0)]])
    assert vote_baseline(I, D, slice(0, 1), "q0", REF, N_DUMMY) == ["a", "b", "c"]
    I, D = _ID([[(14, 2.0), (12, 2.0), (10, 1.0), (11, 1.0)]])
    assert vote_baseline(I, D, slice(0, 1), "q0", REF, N_DUMMY) == ["a", "b", "c"]


def test_vote_sums_in_fp32():
    from neuralsampleid_amd.baseline_eval import vote_baseline
    # a (ids 10, 11, 16): 2^24 + 1 + 1 stays 2^24 in fp32, each 1 is lost; b (ids 12, 13): 2^24 + 2 is exact. fp32: b first; in
    # fp64 the two would tie and a, met first, would lead
    big = float(2 ** 24)
    I, D = _ID([[(10, big), (11, 1.0), (16, 1.0), (12, big), (13, 2.0)]])
    assert vote_baseline(I, D, slice(0, 1), "q0", REF + ["a"], N_DUMMY) == ["b", "a"]


def test_hit_rates_song_missing_from_gt_is_no_hit():
    from neuralsampleid_amd.baseline_eval import hit_rates_baseline
    lookup = ["q0_0", "q0_0", "q1_1"]
    I, D = _ID([[(10, 1.0)], [(12, 3.0)], [(14, 1.0)]])
    gt = {"a": ["q0"], "b": []}                     # c is missing
    hr, raw, ids = hit_rates_baseline(I, D, lookup, REF, N_DUMMY, gt, "1 2")
    assert ids.tolist() == [0, 2] and raw.shape == (2, 6) and raw.dtype == np.int_
    # q0: length 1 -> [a] hit; length 2 -> [b, a]: top-1 miss, top-3 hit. q1: [c], not in gt -> no hit, length 2 not valid
    assert raw.tolist() == [[1, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]]
    np.testing.assert_array_equal(hr, [[50.0, 0.0], [50.0, 100.0], [50.0, 100.0]])


def test_map_skips_short_tests_and_overwrites_a_repeated_query_id():
    from neuralsampleid_amd.baseline_eval import MAP_MIN_ROWS, predictions_baseline
    assert MAP_MIN_ROWS == 10
    lookup = ["q0_0"] * 11 + ["q1_1"] * 10 + ["q0_2"] * 12
    rows = [[(10, 1.0)]] * 11 + [[(12, 1.0)]] * 10 + [[(14, 1.0)]] * 11 + [[(12, 5.0)]]
    I, D = _ID(rows)
    pred = predictions_baseline(I, D, lookup, REF, N_DUMMY)
    assert pred == {"q0": ["b", "c"]}                # q1 has 10 rows: skipped; the second q0 test replaces the first ([a])


def test_argument_checks(tmp_path):
    from neuralsampleid_amd import baseline_eval as be
    from neuralsampleid_amd.fpdb import write_fp_db
    I, D = _ID([[(10, 1.0)], [(12, 3.0)]])
    with pytest.raises(ValueError, match="empty"):
        be.hit_rates_baseline(I[:0], D[:0], [], REF, N_DUMMY, {}, "1")
    with pytest.raises(ValueError, match="empty"):
        be.predictions_baseline(I[:0], D[:0], [], REF, N_DUMMY)
    with pytest.raises(ValueError, match="empty"):
        be.hit_rates_baseline(I, D, ["q0_0", "q0_0"], [], 0, {}, "1")
    with pytest.raises(ValueError, match="one row per query segment"):
        be.hit_rates_baseline(I, D[:, :0], ["q0_0", "q0_0"], REF, N_DUMMY, {}, "1")
    with pytest.raises(ValueError, match="one row per query segment"):
        be.predictions_baseline(I, D, ["q0_0"], REF, N_DUMMY)
    emb = str(tmp_path)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k_probe"):
            be.eval_hit_rates_baseline(emb, {}, k_probe=k)
        with pytest.raises(ValueError, match="k_probe"):
            be.eval_map_baseline(emb, {}, k_probe=k)
    # mismatched d is refused before anything goes to the GPU
    for name, d in (("query_db", 2048), ("query_full_db", 2048), ("ref_db", 1024), ("dummy_db", 2048)):
        write_fp_db(emb, name, np.zeros((2, d), np.float32), ["x_0"] * 2)
    with pytest.raises(ValueError, match="dimension mismatch"):
        be.eval_hit_rates_baseline(emb, {}, save=False)
    with pytest.raises(ValueError, match="dimension mismatch"):
        be.eval_map_baseline(emb, {}, save=False)
