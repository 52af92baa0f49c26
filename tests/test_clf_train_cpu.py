"""Host-side parts of the classifier training loop (neuralsampleid_amd/downstream.py): the pair lists against the reference's own
expressions (downstream.py:123-126) on index tensors, the mining tie rule restated on the host, and the refusals that fire before
the device."""
import numpy as np
import pytest
import torch


def test_pair_lists_match_reference_expressions():
    from neuralsampleid_amd.downstream import pair_lists
    rng = np.random.default_rng(0)
    for B, k in ((1, 1), (2, 3), (8, 3), (32, 5)):
        hn = torch.from_numpy(rng.integers(0, 2 * B, size=(B, k)))
        q_idx, c_idx = pair_lists(hn, B)
        # the reference's tensors, with each segment replaced by its index: x_i = arange(B), x_all = arange(2B)
        x_i = torch.arange(B).view(B, 1, 1)
        x_all = torch.arange(2 * B).view(2 * B, 1, 1)
        x_j = x_all[B:]
        pos_q, pos_c = x_i, x_j                                          # classifier(x_before_proj_i, x_before_proj_j)
        neg_q, neg_c = x_i.repeat(k, 1, 1), x_all[hn.view(-1)]           # classifier(x_i.repeat(3, 1, 1), hard_negatives)
        assert torch.equal(q_idx, torch.cat([pos_q, neg_q]).view(-1))
        assert torch.equal(c_idx, torch.cat([pos_c, neg_c]).view(-1))
        assert q_idx.dtype == c_idx.dtype == torch.int64


def test_pair_lists_query_is_not_the_anchor():
    """negative p pairs x_i[p mod B] with a candidate mined for anchor p // k: they differ (the reference's quirk, kept)"""
    from neuralsampleid_amd.downstream import pair_lists
    B, k = 4, 3
    hn = torch.arange(B * k).view(B, k) % (2 * B)
    q_idx, c_idx = pair_lists(hn, B)
    anchors = torch.arange(B).repeat_interleave(k)
    assert not torch.equal(q_idx[B:], anchors)
    assert torch.equal(q_idx[B:], torch.arange(B * k) % B)


def test_pair_lists_refuse_bad_shapes():
    from neuralsampleid_amd.downstream import pair_lists
    with pytest.raises(ValueError):
        pair_lists(torch.zeros(3, 2, dtype=torch.int64), 4)
    with pytest.raises(ValueError):
        pair_lists(torch.zeros(6, dtype=torch.int64), 2)


def host_mine(z_i, z_all, k):
    """the tie rule restated: ranks 1..k of the descending order of fp32 dots (sequential fma chains), ties to the smaller index"""
    sim = np.array([[np.float32(0)] * z_all.shape[0]] * z_i.shape[0], dtype=np.float32)
    for i in range(z_i.shape[0]):
        for j in range(z_all.shape[0]):
            acc = np.float32(0)
            for e in range(z_i.shape[1]):
                acc = np.float32(acc + np.float32(z_i[i, e] * z_all[j, e]))
            sim[i, j] = acc
    order = np.lexsort((np.tile(np.arange(z_all.shape[0]), (z_i.shape[0], 1)), -sim), axis=1)
    return order[:, 1:k + 1]


def test_tie_rule_on_duplicates():
    rng = np.random.default_rng(1)
    B, d = 6, 8
    z_i = rng.integers(-2, 3, size=(B, d)).astype(np.float32)      # small integers: exact dots, many ties
    z_j = z_i.copy()
    z_j[2] = z_i[4]
    z_all = np.concatenate([z_i, z_j])
    hn = host_mine(z_i, z_all, 3)
    for i in range(B):
        sim = z_all @ z_i[i]
        expect = sorted(range(2 * B), key=lambda j: (-sim[j], j))[1:4]
        assert list(hn[i]) == expect
    # row 4 equals rows 4, 8 (= z_j[2]) and 10: rank 0 is 4 itself, then 8 and 10 in index order
    assert list(hn[4][:2]) == [8, 10]
    # argsort's own order is not defined for ties; the stable descending sort is the rule
    assert np.array_equal(hn, np.argsort(-(z_i @ z_all.T), axis=1, kind="stable")[:, 1:4])


def test_refusals_before_the_device():
    from neuralsampleid_amd import downstream
    with pytest.raises(ValueError):
        downstream.draw_keep(4, 1.0, "cpu")
    with pytest.raises(ValueError):
        downstream.draw_keep(4, -0.5, "cpu")
    z = torch.randn(4, 128)
    with pytest.raises(ValueError):                     # CPU tensors: the miner runs on the MI355X only
        downstream.mine_hard_negatives(z, z, torch.cat([z, z]))
    with pytest.raises(ValueError):
        downstream.mine_hard_negatives(z.double(), z, torch.cat([z, z]))


def test_train_scores_refuses_cpu_and_grad_inputs():
    from neuralsampleid_amd import downstream
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    clf = CrossAttentionClassifier(512, num_nodes=32)
    x = torch.randn(2, 512, 8)
    keep = torch.ones(2, 128)
    with pytest.raises(RuntimeError):
        downstream.clf_train_scores(clf, x, x, [0, 1], [1, 0], keep)
    with pytest.raises(ValueError):
        downstream.clf_train_scores(clf, x.double(), x, [0, 1], [1, 0], keep)
    with pytest.raises(NotImplementedError):
        downstream.clf_train_scores(CrossAttentionClassifier(512, num_heads=8, num_nodes=32), x, x, [0, 1], [1, 0], keep)
    with pytest.raises(NotImplementedError):
        downstream.clf_train_scores(CrossAttentionClassifier(256, num_nodes=32), x, x, [0, 1], [1, 0], keep)
