"""GPU: the classifier re-rank pair scores (csrc/rerank.hip via classifier.CrossAttentionClassifier) against an fp64
nn.MultiheadAttention classifier, their invariances and argument checks, and eval_hit_rates_clf / eval_map_clf against the golden
made by the reference's own eval_faiss_clf / eval_faiss_map_clf (tests/golden/make_rerank_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# input scale of every parity test: node matrices ~ N(0, 1) (the pre-projection nodes of the encoder are O(1)); weights by the
# golden's rule (classifier_state: in_proj / out_proj ~ N(0, 1/512), fc.0 ~ N(0, 16/512), fc.3 ~ N(0, 16/128))
TOL = 1e-5


def _classifier(seed=3, pos_embed=True, b2=0.0):
    from make_rerank_golden import classifier_state
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    sd = classifier_state(seed, b2)
    if not pos_embed:
        del sd["positional_embedding"]
    clf = CrossAttentionClassifier(in_dim=512, num_nodes=32, pos_embed=pos_embed)
    clf.load_state_dict(sd, strict=True)
    return clf.to(DEV).eval(), sd


def _fp64(sd):
    from make_rerank_golden import fp64_classifier
    return fp64_classifier(sd).to(DEV)


def _ref_scores(model, q, c, batch=512):
    """(Sq, C, N) x (Sc, C, N) -> (Sq, Sc) fp64 on the GPU"""
    q64, c64 = q.to(DEV, torch.float64), c.to(DEV, torch.float64)
    Sq, Sc = q.shape[0], c.shape[0]
    qi = torch.arange(Sq * Sc, device=DEV) // Sc
    ci = torch.arange(Sq * Sc, device=DEV) % Sc
    out = torch.empty(Sq * Sc, device=DEV, dtype=torch.float64)
    with torch.no_grad():
        for a in range(0, Sq * Sc, batch):
            out[a:a + batch] = model(q64[qi[a:a + batch]], c64[ci[a:a + batch]])[:, 0]
    return out.view(Sq, Sc)


def _nodes(g, S, N):
    return torch.randn(S, 512, N, generator=g).to(DEV)


@pytest.mark.parametrize("Sq,Sc,N,pos", [(1, 1, 32, True), (31, 33, 32, True), (32, 300, 32, False), (33, 32, 20, True),
                                         (300, 31, 32, True), (33, 1, 7, False)])
def test_pair_scores_vs_fp64(Sq, Sc, N, pos):
    clf, sd = _classifier(pos_embed=pos)
    g = torch.Generator().manual_seed(Sq * 1000 + Sc + N)
    q, c = _nodes(g, Sq, N), _nodes(g, Sc, N)
    with torch.no_grad():
        got = clf.pair_scores(q, c)
    ref = _ref_scores(_fp64(sd), q, c)
    assert got.shape == (Sq, Sc) and got.dtype == torch.float32
    err = float((got.double() - ref).abs().max())
    assert err <= TOL, err
    if Sc > 1:                                   # the scores are not all the same (they vary mostly with the candidate)
        assert float(ref.std()) > 1e-3


def test_candidate_lists_with_repeats_and_groups():
    """several groups in one call, unsorted candidate lists with repeats: every block equals the fp64 scores of its pairs"""
    clf, sd = _classifier()
    g = torch.Generator().manual_seed(11)
    q, c = _nodes(g, 70, 32), _nodes(g, 40, 32)
    rng = np.random.default_rng(0)
    lists = [rng.integers(0, 40, size=n) for n in (5, 33, 1, 64)]
    lists[0][:] = [3, 3, 0, 39, 3]
    qs, qn = [0, 10, 69, 2], [10, 66 - 10, 1, 65]
    with torch.no_grad():
        qp, kp = clf.project_queries(q), clf.project_candidates(c)
        out, off = clf.score_blocks(qp, kp, 32, qs, qn, np.concatenate(lists), np.cumsum([0] + [len(x) for x in lists[:-1]]),
                                    [len(x) for x in lists])
    ref = _ref_scores(_fp64(sd), q, c)
    for i, lst in enumerate(lists):
        blk = out[off[i]:off[i] + qn[i] * len(lst)].view(qn[i], len(lst)).double()
        want = ref[qs[i]:qs[i] + qn[i]][:, torch.as_tensor(lst, device=DEV)]
        assert float((blk - want).abs().max()) <= TOL


def test_forward_pairs_vs_fp64():
    clf, sd = _classifier()
    g = torch.Generator().manual_seed(5)
    x_i, x_j = _nodes(g, 48, 32), _nodes(g, 48, 32)
    with torch.no_grad():
        got = clf(x_i, x_j)
        ref = _fp64(sd)(x_i.double(), x_j.double())
    assert got.shape == (48, 1)
    assert float((got.double() - ref).abs().max()) <= TOL


def test_bitwise_invariance_and_run_to_run():
    clf, _ = _classifier()
    g = torch.Generator().manual_seed(9)
    q, c = _nodes(g, 200, 32), _nodes(g, 150, 32)
    with torch.no_grad():
        qp, kp = clf.project_queries(q), clf.project_candidates(c)
        rng = np.random.default_rng(1)
        lists = [rng.integers(0, 150, size=n) for n in (150, 7, 90)]
        qs, qn = [0, 100, 37], [200, 100, 130]
        args = (qp, kp, 32, qs, qn, np.concatenate(lists), np.cumsum([0] + [len(x) for x in lists[:-1]]), [len(x) for x in lists])
        big, off = clf.score_blocks(*args)
        again, _ = clf.score_blocks(*args)
        assert torch.equal(big, again)
        for (gi, qi, cj) in ((0, 0, 0), (0, 199, 149), (1, 5, 3), (2, 129, 89), (2, 64, 0)):
            alone, _ = clf.score_blocks(qp, kp, 32, [qs[gi] + qi], [1], [lists[gi][cj]], [0], [1])
            assert torch.equal(alone[0], big[off[gi] + qi * len(lists[gi]) + cj]), (gi, qi, cj)
        # projections are row-invariant too: a pair scored through pair_scores alone equals its entry in the full matrix
        full = clf.pair_scores(q, c)
        one = clf.pair_scores(q[17:18].contiguous(), c[101:102].contiguous())
        assert torch.equal(one[0, 0], full[17, 101])


def test_refusal_before_launch():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    clf, _ = _classifier()
    x = torch.randn(4, 512, 32, device=DEV)
    bad = [torch.randn(4, 256, 32, device=DEV), torch.randn(4, 512, 33, device=DEV), x.double(), x.half(),
           torch.randn(4, 32, 512, device=DEV).transpose(1, 2)]
    ops.launch_counters(reset=True)
    with torch.no_grad():
        for b in bad:
            with pytest.raises(ValueError):
                clf.pair_scores(b, b)
            with pytest.raises(ValueError):
                clf(b, b)
        with pytest.raises(ValueError):
            clf.pair_scores(x, torch.randn(4, 512, 16, device=DEV))
        for kw in ({"num_heads": 8}, {"hidden_dim": 64}):
            other = CrossAttentionClassifier(in_dim=512, num_nodes=32, **kw).to(DEV).eval()
            with pytest.raises(NotImplementedError):
                other.pair_scores(x, x)
        other = CrossAttentionClassifier(in_dim=256, num_nodes=32).to(DEV).eval()
        with pytest.raises(NotImplementedError):
            other.pair_scores(torch.randn(2, 256, 32, device=DEV), torch.randn(2, 256, 32, device=DEV))
    with pytest.raises(NotImplementedError, match="training"):
        clf.pair_scores(x, x)                       # grad enabled
    clf.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training"):
        clf(x, x)                                   # training mode
    clf.eval()
    c = ops.launch_counters()
    assert sum(c.values()) == 0, {k: v for k, v in c.items() if v}
    with torch.no_grad():
        qp, kp = clf.project_queries(x), clf.project_candidates(x)
    ops.launch_counters(reset=True)
    with torch.no_grad():
        for args in (([0], [5], [0], [0], [1]), ([0], [1], [4], [0], [1]), ([0], [1], [-1], [0], [1]), ([0], [1], [0], [0], [2])):
            with pytest.raises(ValueError):
                clf.score_blocks(qp, kp, 32, *args)
        with pytest.raises(ValueError):
            ops.clf_pair_scores(qp, kp, 33, clf.folded()[4], [0], [1], [0], [0], [1])
    c = ops.launch_counters()
    assert c["clf_pair_scores"] == 0 and c["clf_node_rows"] == 0 and sum(c.values()) == 0, {k: v for k, v in c.items() if v}


# ------------------------------------------------------------------------------------------------ the reference-made golden
def _file_digests(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def test_evaluations_match_reference_golden(tmp_path):
    from make_rerank_golden import load_golden_inputs, write_inputs
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.rerank import eval_hit_rates_clf, eval_map_clf
    z, inp, state = load_golden_inputs()
    p = json.loads(bytes(z["params"]).decode())
    emb = str(tmp_path / "emb")
    write_inputs(inp, emb)
    gt_path = str(tmp_path / "gt_dict.json")
    with open(gt_path, "w") as f:
        json.dump(inp["gt"], f)
    clf = CrossAttentionClassifier(in_dim=512, num_nodes=p["num_nodes"])
    clf.load_state_dict(state, strict=True)
    clf = clf.to(DEV).eval()
    before = _file_digests(emb)
    hr = eval_hit_rates_clf(emb, clf, gt_path, test_seq_len=p["test_seq_len"], k_probe=p["k_probe"])
    m, k = eval_map_clf(emb, clf, gt_path, k_probe=p["k_map_probe"], k_map=p["k_map"])
    after = _file_digests(emb)
    for f, h in before.items():
        assert after[f] == h, f"{f} was modified"
    assert set(after) - set(before) == {"hit_rates_clf.npy", "raw_score_clf.npy", "test_ids_clf.npy", "predictions.npy",
                                        "map_score.npy"}
    np.testing.assert_array_equal(hr, z["hit_rates"])
    for name, fname in (("hit_rates", "hit_rates_clf"), ("raw_score", "raw_score_clf"), ("test_ids", "test_ids_clf"),
                        ("map_score", "map_score")):
        got = np.load(os.path.join(emb, fname + ".npy"))
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])
    assert k == p["k_map"] and float(m) == float(z["map_score"])
    pred = np.load(os.path.join(emb, "predictions.npy"), allow_pickle=True).item()
    assert pred == json.loads(bytes(z["predictions"]).decode())


def test_end_to_end_extract_node_matrices_and_evaluate(tmp_path):
    from neuralsampleid_amd import fpdb
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.encoder.dgl.graph_encoder import GraphEncoderDGL
    from neuralsampleid_amd.rerank import eval_hit_rates_clf, eval_map_clf
    from neuralsampleid_amd.simclr.simclr import SimCLR
    from synth import GRAFP_CFG, synth_clips, synth_state
    torch.manual_seed(0)
    model = SimCLR(GRAFP_CFG, GraphEncoderDGL(cfg=GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict(), ""))
    model = model.to(DEV).eval()
    x, _ = synth_clips(24)
    x = x.to(DEV)
    songs = [(f"song{i}", x[4 * i:4 * i + 4]) for i in range(6)]
    queries = [(f"q{i}", x[4 * i + 1:4 * i + 3]) for i in (1, 3, 4)]
    emb = str(tmp_path / "emb")
    fpdb.build_fp_db(model, songs, emb, "ref_db", batch=8)
    fpdb.build_fp_db(model, songs[:1], emb, "dummy_db", batch=8)
    fpdb.build_fp_db(model, queries, emb, "query_db", query_style=True, batch=8)
    fpdb.build_fp_db(model, queries, emb, "query_full_db", batch=8)
    shapes = fpdb.build_node_matrices(model, songs, os.path.join(emb, "ref_nmatrix"), batch=8)
    fpdb.build_query_node_matrices(model, queries, os.path.join(emb, "query_nmatrix.npy"), batch=8)
    fpdb.build_query_node_matrices(model, queries, os.path.join(emb, "query_full_nmatrix.npy"), batch=8)
    assert shapes["song0"] == (4, 512, 32)
    with torch.no_grad():
        want, _ = model.encoder(model.peak_extractor(x[:4]), return_pre_proj=True)
    got = np.load(os.path.join(emb, "ref_nmatrix", "song0.npy"))
    assert got.dtype == np.float32
    torch.testing.assert_close(torch.from_numpy(got), want.cpu(), rtol=1e-6, atol=1e-6)
    qnm = np.load(os.path.join(emb, "query_nmatrix.npy"), allow_pickle=True).item()
    assert list(qnm) == ["q1", "q3", "q4"] and qnm["q3"].shape == (2, 512, 32)
    clf, _ = _classifier(seed=1)
    gt = {f"song{i}": ([f"q{i}"] if i in (1, 3, 4) else []) for i in range(6)}
    hr = eval_hit_rates_clf(emb, clf, gt, test_seq_len="1 2", k_probe=3, save=False)
    assert hr.shape == (3, 2) and np.isfinite(hr).all()
    m, k = eval_map_clf(emb, clf, gt, k_probe=3, save=False)
    assert k == 20 and 0.0 <= float(m) <= 1.0
