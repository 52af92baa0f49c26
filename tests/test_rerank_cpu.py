"""CPU: the host side of the classifier re-rank evaluation (neuralsampleid_amd.rerank / classifier) — state_dict layout, calculate_map,
the two song votes rule by rule, and a replay of the golden made by the reference's own eval_faiss_clf / eval_faiss_map_clf."""
import json

import numpy as np
import pytest
import torch
import torch.nn as nn


def _reference_layout(in_dim=512, num_nodes=32, pos_embed=True):
    m = nn.Module()
    if pos_embed:
        m.register_buffer("positional_embedding", torch.randn(1, num_nodes, in_dim))
    m.attn = nn.MultiheadAttention(embed_dim=in_dim, num_heads=4, batch_first=True)
    m.fc = nn.Sequential(nn.Linear(in_dim, 128), nn.ReLU(), nn.Dropout(p=0.3), nn.Linear(128, 1), nn.Sigmoid())
    return m


@pytest.mark.parametrize("pos_embed", [True, False])
def test_state_dict_matches_reference_layout(pos_embed):
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    ref = _reference_layout(pos_embed=pos_embed)
    ours = CrossAttentionClassifier(in_dim=512, num_nodes=32, pos_embed=pos_embed)
    a, b = ref.state_dict(), ours.state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape for k in a)
    ours.load_state_dict(a, strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert all(torch.equal(ours.state_dict()[k], a[k]) for k in a)


def test_forward_refuses_training_and_grad():
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    clf = CrossAttentionClassifier(in_dim=512, num_nodes=32)
    x = torch.zeros(2, 512, 32)
    with pytest.raises(NotImplementedError, match="training"):
        clf(x, x)                                   # training mode
    clf.eval()
    with pytest.raises(NotImplementedError, match="training"):
        clf(x, x)                                   # grad enabled


def test_calculate_map_hand_cases():
    from neuralsampleid_amd.rerank import calculate_map
    gt = {"a": ["q1"], "b": ["q1", "q2"], "c": []}
    assert calculate_map(gt, {"q1": ["a", "x", "b"]}, k=20) == pytest.approx((1 / 1 + 2 / 3) / 2)
    assert calculate_map(gt, {"q1": ["x", "a"]}, k=1) == 0           # the hit is past k
    assert calculate_map(gt, {"q1": ["c", "zz"], "q2": ["b"]}, k=20) == pytest.approx(0.5)   # missing song: not relevant
    assert calculate_map(gt, {}, k=20) == 0
    # not divided by the number of relevant items: one hit of two relevant at rank 1 -> 1.0
    assert calculate_map({"a": ["q"], "b": ["q"]}, {"q": ["a", "x"]}, k=20) == 1.0


REF = ["a", "a", "a", "b", "b", "qx", "c"]      # runs: a 0-2, b 3-4, qx 5, c 6
ND = 2                                           # ids 0, 1 are dummies; ref id r is cid r + 2


def _scores(cands, S):
    return (np.asarray(cands, np.int64), np.asarray(S, np.float64))


def test_hit_rate_vote_rules():
    from neuralsampleid_amd.rerank import vote_hit_rates_clf
    ref_rows = {"a": 3, "b": 1, "qx": 1}         # c: no file; b: segment 1 is past its one row
    # walk: -1, dummy 0, own song qx (7), b seg 1 (6: out of bounds), c (8: missing), a seg 0 (2), b seg 0 (5), a seg 0 again (2)
    I = np.array([[-1, 0, 7, 6], [8, 2, 5, 2]])
    cands = [2, 5]
    S = [[0.6, 0.9], [0.7, 0.2]]                 # rows = query segments; sl = 1 uses row 0 only
    gt = {"a": ["qx"], "b": []}
    hr, raw, tid, skips = vote_hit_rates_clf(I, [_scores(cands, S)], ["qx_0", "qx_0"], REF, ND, gt, ref_rows, "1 2")
    # sl = 1: row 0 only -> nothing counted: no prediction, no hit
    # sl = 2: a = 0.7 + 0.7 (duplicate adds again), b = 0.9 -> a first
    assert raw.tolist() == [[0, 1, 0, 1, 0, 1]] and tid.tolist() == [0]
    assert skips == (1, 2)                       # (missing, out of bounds) over both walks: c at sl = 2, b1 at sl = 1 and 2
    S = [[0.4, 0.9], [0.49, 0.95]]               # a's max over the first 2 rows is below 0.5 -> not added; b = 0.95
    _, raw, _, _ = vote_hit_rates_clf(I, [_scores(cands, S)], ["qx_0", "qx_0"], REF, ND, gt, ref_rows, "2")
    assert raw.tolist() == [[0, 0, 0]]
    S = [[0.4, 0.9], [0.5, 0.5]]                 # exactly 0.5 enters; a (0.5 + 0.5) before b (0.9)
    _, raw, _, _ = vote_hit_rates_clf(I, [_scores(cands, S)], ["qx_0", "qx_0"], REF, ND, gt, ref_rows, "2")
    assert raw.tolist() == [[1, 1, 1]]
    # ties in first-appearance order: a appears before b in the walk
    I2 = np.array([[2, 5]])
    gt2 = {"a": [], "b": ["qx"]}
    _, raw, _, _ = vote_hit_rates_clf(I2, [_scores(cands, [[0.8, 0.8]])], ["qx_0"], REF, ND, gt2, ref_rows, "1")
    assert raw.tolist() == [[0, 1, 1]]
    # a predicted song missing from gt is no hit (the reference would raise KeyError)
    _, raw, _, _ = vote_hit_rates_clf(I2, [_scores(cands, [[0.8, 0.8]])], ["qx_0"], REF, ND, {}, ref_rows, "1")
    assert raw.tolist() == [[0, 0, 0]]


def test_map_vote_rules():
    from neuralsampleid_amd.rerank import calculate_map, vote_map_clf
    ref_rows = {"a": 3, "b": 2, "qx": 1, "c": 1}
    # unique ascending candidates, frequencies ignored: 2 (a0), 3 (a1), 5 (b0), 6 (b1), 7 (own song), 8 (c0), dummy 1
    I = np.array([[8, 5, 1], [2, 2, 7], [3, 6, -1]])
    cands = [2, 3, 5, 6, 8]
    S = [[0.2, 0.3, 0.4, 0.45, 0.1], [0.1, 0.2, 0.3, 0.4, 0.2]]    # everything <= 0.5: every song enters at 0
    pred, _ = vote_map_clf(I, [_scores(cands, S)], ["qx"] * 3, REF, ND, ref_rows)
    assert pred == {"qx": ["a", "b", "c"]}           # ties at 0 in insertion order = ascending candidate id
    S = [[0.2, 0.3, 0.4, 0.45, 0.5], [0.1, 0.2, 0.3, 0.51, 0.2]]    # 0.5 does not count (strict), 0.51 does
    pred, _ = vote_map_clf(I, [_scores(cands, S)], ["qx"] * 3, REF, ND, ref_rows)
    assert pred == {"qx": ["b", "a", "c"]}
    # a repeated q_id overwrites its prediction and keeps its dict position
    I3 = np.array([[2], [5], [8]])
    pred, _ = vote_map_clf(I3, [_scores([2], [[0.9]]), _scores([5], [[0.9]]), _scores([8], [[0.9]])], ["qx", "qy", "qx"], REF, ND,
                           ref_rows)
    assert list(pred) == ["qx", "qy"] and pred["qx"] == ["c"] and pred["qy"] == ["b"]
    assert calculate_map({"c": ["qx"]}, pred, 20) == 0.5
    # missing file / out of bounds are skipped
    pred, skips = vote_map_clf(I, [_scores([2, 3, 5], [[0.9, 0.9, 0.9]])], ["qx"] * 3, REF, ND, {"a": 1, "b": 1})
    assert pred == {"qx": ["a", "b"]} and skips == (1, 2)


def test_golden_replay_on_fp64_scores():
    """the fixture's I and fp64 scores of an nn.MultiheadAttention classifier with the rule weights: the host votes reproduce the
    reference's hit_rates, raw_score, test_ids, map_score and predictions exactly"""
    from make_rerank_golden import fp64_classifier, host_scores, load_golden_inputs
    from neuralsampleid_amd.rerank import calculate_map, vote_hit_rates_clf, vote_map_clf
    z, inp, state = load_golden_inputs()
    p = json.loads(bytes(z["params"]).decode())
    model = fp64_classifier(state)
    I_hr, I_map = z["I_hr"].astype(np.int64), z["I_map"].astype(np.int64)
    nd = inp["dummy"].shape[0]
    scores, ref_rows = host_scores(inp, I_hr, model, p, False)
    hr, raw, tid, skips = vote_hit_rates_clf(I_hr, scores, inp["query_lookup"], inp["ref_lookup"], nd, inp["gt"], ref_rows,
                                             p["test_seq_len"])
    for got, name in ((hr, "hit_rates"), (raw, "raw_score"), (tid, "test_ids")):
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])
    assert skips[0] > 0 and skips[1] > 0
    scores, ref_rows = host_scores(inp, I_map, model, p, True)
    pred, _ = vote_map_clf(I_map, scores, inp["query_full_lookup"], inp["ref_lookup"], nd, ref_rows)
    assert pred == json.loads(bytes(z["predictions"]).decode())
    m = calculate_map(inp["gt"], pred, p["k_map"])
    assert np.asarray(m).dtype == z["map_score"].dtype and float(m) == float(z["map_score"])
    assert 0 < float(m) < 1
