"""CPU: the host side of the exact-mode evaluation (neuralsampleid_amd.search) — the song-level vote against the golden made by
the reference's own eval_faiss, test-start extraction, and argument checks."""
import numpy as np
import pytest


def test_aggregation_reproduces_reference_golden():
    """given the golden's I and fp64 sequence scores, the host vote reproduces raw_score, hit_rates and test_ids exactly"""
    import json
    from make_search_golden import load_golden_inputs, sequence_scores
    from neuralsampleid_amd.search import aggregate_hit_rates, extract_test_ids
    z, inp = load_golden_inputs()
    p = json.loads(bytes(z["params"]).decode())
    I = z["I"].astype(np.int64)
    xb = np.concatenate([inp["dummy"], inp["ref"]])
    starts, lens = extract_test_ids(inp["query_lookup"])
    scores = sequence_scores(I, inp["query"], xb, starts, lens, p["test_seq_len"], p["k_probe"])
    hr, raw, tid = aggregate_hit_rates(I, scores, inp["query_lookup"], inp["ref_lookup"], inp["dummy"].shape[0], inp["gt"],
                                       p["test_seq_len"])
    for got, name in ((hr, "hit_rates"), (raw, "raw_score"), (tid, "test_ids")):
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])
    assert 0 < hr[0, 0] < 100            # the fixture is not trivial


def test_aggregation_rules():
    """dummy ids, -1 and the query's own name are skipped; duplicates add again; ties keep first-appearance order"""
    from neuralsampleid_amd.search import aggregate_hit_rates
    ref_lookup = ["a", "b", "c", "qx"]
    query_lookup = ["qx_0"]
    n_dummy = 2
    # walk order: dummy 0, -1, own name "qx" (id 5), b (3), a (2), b (3)  -> a: 1.0, b: 0.5 + 0.5 = 1.0: tie, b appeared first
    I = np.array([[0, -1, 5, 3, 2, 3]])
    scores = np.array([[9.0, np.nan, 9.0, 0.5, 1.0, 0.5]])
    gt = {"a": [], "b": ["qx"], "c": ["qx"]}
    hr, raw, tid = aggregate_hit_rates(I, scores, query_lookup, ref_lookup, n_dummy, gt, "1 3")
    assert raw.tolist() == [[1, 0, 1, 0, 1, 0]] and tid.tolist() == [0]
    assert hr[:, 0].tolist() == [100.0, 100.0, 100.0] and np.isnan(hr[:, 1]).all()
    gt = {"a": ["qx"], "b": [], "c": []}                 # a is second: top-3 but not top-1
    _, raw, _ = aggregate_hit_rates(I, scores, query_lookup, ref_lookup, n_dummy, gt, "1")
    assert raw.tolist() == [[0, 1, 1]]
    _, raw, _ = aggregate_hit_rates(np.array([[0, 1, -1, 0, 1, 1]]), scores, query_lookup, ref_lookup, n_dummy, gt, "1")
    assert raw.tolist() == [[0, 0, 0]]                  # only dummies: no prediction, no hit


def test_extract_test_ids_edge_cases():
    from neuralsampleid_amd.search import extract_test_ids
    s, l = extract_test_ids(["x_0"] * 7)                # one song
    assert s.tolist() == [0] and l.tolist() == [7] and s.dtype == np.int64
    names = [f"q{i}_{i}" for i in range(5)]             # all distinct
    s, l = extract_test_ids(names)
    assert s.tolist() == [0, 1, 2, 3, 4] and l.tolist() == [1] * 5
    s, l = extract_test_ids(["a", "a", "b", "a"])       # a name that comes back is a new test
    assert s.tolist() == [0, 2, 3] and l.tolist() == [2, 1, 1]
    with pytest.raises(ValueError):
        extract_test_ids([])


def test_make_pairs_limits_lengths():
    from neuralsampleid_amd.search import make_pairs
    ti, si, ps, pl = make_pairs([0, 4, 5], [4, 1, 12], "1 3 5 9 11 19")
    assert ti.tolist() == [0, 0, 1, 2, 2, 2, 2, 2] and pl.tolist() == [1, 3, 1, 1, 3, 5, 9, 11]
    assert ps.tolist() == [0, 0, 4, 5, 5, 5, 5, 5] and si.tolist() == [0, 1, 0, 0, 1, 2, 3, 4]


def test_host_argument_checks():
    from neuralsampleid_amd.search import aggregate_hit_rates, parse_seq_len
    with pytest.raises(ValueError):
        parse_seq_len("0 3")
    with pytest.raises(ValueError):
        parse_seq_len([])
    assert parse_seq_len("1 3 5").tolist() == [1, 3, 5] and parse_seq_len([2, 4]).tolist() == [2, 4]
    I = np.zeros((2, 3), np.int64)
    with pytest.raises(ValueError):                     # I has a row per query segment
        aggregate_hit_rates(I, np.zeros((1, 3)), ["q_0"] * 3, ["a"], 0, {}, "1")
    with pytest.raises(ValueError):                     # scores too narrow for length 2 x k 3
        aggregate_hit_rates(I, np.zeros((2, 5)), ["q_0"] * 2, ["a"], 0, {}, "1 2")
    with pytest.raises(ValueError):
        aggregate_hit_rates(I, np.zeros((1, 3)), ["q_0"] * 2, ["a"], -1, {}, "1")


def test_eval_entry_checks_before_any_gpu_work(tmp_path):
    """eval_hit_rates / FlatL2Index refuse bad arguments up front (these checks run without a GPU)"""
    from neuralsampleid_amd.search import FlatL2Index, eval_hit_rates
    with pytest.raises(ValueError):
        eval_hit_rates(str(tmp_path), {}, k_probe=0)
    with pytest.raises(ValueError):
        eval_hit_rates(str(tmp_path), {}, k_probe=65)
    with pytest.raises(TypeError):
        eval_hit_rates(str(tmp_path), ["not", "a", "dict"])
    with pytest.raises(ValueError):
        FlatL2Index(100)
    with pytest.raises(RuntimeError):
        FlatL2Index(128, "cpu")


def test_workspace_query_for_search():
    from neuralsampleid_amd._lib import lib
    a = lib.nsid_workspace_bytes(b"flat_l2_topk", 16384, 1 << 20)
    b = lib.nsid_workspace_bytes(b"flat_l2_topk", 19, 1 << 20)
    assert a > 0 and b > 0 and a % (16384 * 64 * 8) == 0 and b % (19 * 64 * 8) == 0
    assert lib.nsid_workspace_bytes(b"flat_l2_topk", 5, 0) == 5 * 64 * 8
