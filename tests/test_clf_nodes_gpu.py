"""Classifier re-rank for node matrices of 33 .. 128 nodes on the MI355X (clf_pair_wide_kernel of csrc/rerank.hip through
classifier.py and ops.py): parity with an fp64 nn.MultiheadAttention restatement of the reference module at every way the 32 x 32
tiling can go wrong, the reference's own scores and evaluations (tests/golden/clf_nodes.npz), bitwise invariance, reads that stay
inside the data, the untouched N <= 32 path, refusals that launch nothing, and the 256-mel encoder end to end.

The bound 1e-5 (absolute, against fp64) is the project's bound for classifier scores. The reference module's own fp32 against fp64
at these sizes is at most 7.8e-7 (N in {33, 64, 97, 128}, C in {512, 1024}, three seeds, scores spread over [0.02, 0.998]) and
3.1e-7 on the golden's inputs (stored in the fixture, asserted <= 1e-6 by test_clf_nodes_cpu.py), so 1e-5 leaves 10x for another
fixed summation order."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _mods():
    from neuralsampleid_amd import downstream, ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    return downstream, ops, CrossAttentionClassifier


def rule_state(seed, C, num_nodes, pos_embed=True, b2=0.0):
    from make_rerank_golden import classifier_state
    sd = classifier_state(seed, b2, {"C": C, "num_nodes": num_nodes})
    if not pos_embed:
        del sd["positional_embedding"]
    return sd


def make_clf(state, C, num_nodes, pos_embed=True):
    _, _, CAC = _mods()
    clf = CAC(C, num_nodes=num_nodes, pos_embed=pos_embed)
    clf.load_state_dict(state, strict=True)
    return clf.to(DEV).eval()


def fp64_scores(state, q, c, batch=64):
    """(Sq, C, N) x (Sc, C, N) -> (Sq, Sc): the reference module restated in fp64 (make_rerank_golden.fp64_classifier), on the GPU"""
    from make_rerank_golden import fp64_classifier
    model = fp64_classifier(state).to(DEV)
    q64, c64 = q.to(DEV, torch.float64), c.to(DEV, torch.float64)
    Sq, Sc = q.shape[0], c.shape[0]
    idx = torch.arange(Sq * Sc, device=DEV)
    out = torch.empty(Sq * Sc, device=DEV, dtype=torch.float64)
    with torch.no_grad():
        for a in range(0, Sq * Sc, batch):
            out[a:a + batch] = model(q64[idx[a:a + batch] // Sc], c64[idx[a:a + batch] % Sc])[:, 0]
    return out.view(Sq, Sc)


def nodes(seed, S, C, N):
    return torch.randn(S, C, N, generator=torch.Generator().manual_seed(seed)).to(DEV).contiguous()


def clf_counts(ops):
    return {k: v for k, v in ops.launch_counters().items() if k.startswith("clf_")}


# ------------------------------------------------------------------------------------------------ against fp64
# (C, Sq, Sc, N, pos): one key and one query row in the second tile; exact tiles; a partial fourth tile; the full size; 65 query
# segments (the second workgroup of a candidate has one); the other widths at the full size
# fc.3.bias of a case whose rule-made weights would put every score near 1 (logits around 3.5, fp64 on the CPU): centred, so that
# an error in the hidden vector shows in the score at full size
B2 = {(512, 128): -3.5}
CASES = [(512, 3, 2, 33, True), (512, 3, 2, 64, False), (512, 2, 3, 97, True), (512, 5, 4, 128, True), (512, 65, 2, 128, True),
         (640, 3, 2, 128, True), (768, 3, 2, 128, True), (1024, 3, 2, 128, True)]


@pytest.mark.parametrize("C,Sq,Sc,N,pos", CASES)
def test_pair_scores_vs_fp64(C, Sq, Sc, N, pos):
    _, ops, _ = _mods()
    state = rule_state(700 + C + N, C, 128, pos, b2=B2.get((C, N), 0.0))
    clf = make_clf(state, C, 128, pos)
    q, c = nodes(C + N, Sq, C, N), nodes(C + N + 1, Sc, C, N)
    ops.launch_counters(reset=True)
    with torch.no_grad():
        got = clf.pair_scores(q, c)
    cnt = clf_counts(ops)
    ref = fp64_scores(state, q, c)
    err = float((got.double() - ref).abs().max())
    std = float(got.double().std())
    print(f"C {C} {Sq} x {Sc} N {N} pos {pos}: |d| {err:.3g}, scores [{float(got.min()):.4f}, {float(got.max()):.4f}] std {std:.3g}")
    assert got.shape == (Sq, Sc) and got.dtype == torch.float32
    assert cnt["clf_pair_scores_n"] == 1 and cnt["clf_node_rows_n"] == 2 and cnt["clf_pair_scores"] == 0 and cnt["clf_node_rows"] == 0
    assert err < TOL, err
    assert std > 1e-3                           # a constant output cannot pass


def test_forward_pairs_vs_fp64():
    C, N, B = 512, 97, 3
    state = rule_state(41, C, 100)
    clf = make_clf(state, C, 100)
    x_i, x_j = nodes(42, B, C, N), nodes(43, B, C, N)
    with torch.no_grad():
        got = clf(x_i, x_j)
    ref = fp64_scores(state, x_i, x_j).diagonal()
    assert got.shape == (B, 1)
    assert float((got.double().view(-1) - ref).abs().max()) < TOL


# ------------------------------------------------------------------------------------------------ the reference's own numbers
@pytest.fixture(scope="module")
def golden():
    from make_clf_nodes_golden import load_golden_inputs
    return load_golden_inputs()


@pytest.mark.parametrize("case", ["n128", "n70"])
@pytest.mark.parametrize("C", [512, 1024])
def test_reference_golden_scores(golden, C, case):
    z, cases, _ = golden
    p, nm, state = cases[(C, case)]
    clf = make_clf(state, C, p["num_nodes"])
    with torch.no_grad():
        s = clf.pair_scores(torch.from_numpy(nm[0]).to(DEV), torch.from_numpy(nm[1]).to(DEV)).cpu().numpy()
    e = float(np.abs(s.astype(np.float64) - z[f"{C}/{case}/scores"]).max())
    print(f"C {C} {case}: |d| against the reference module {e:.3g}")
    assert e < TOL


def test_evaluations_match_reference_golden(golden, tmp_path):
    from make_rerank_golden import write_inputs
    from neuralsampleid_amd.rerank import eval_hit_rates_clf, eval_map_clf
    _, ops, _ = _mods()
    z, _, (p, inp, state) = golden
    emb = str(tmp_path / "emb")
    write_inputs(inp, emb)
    gt_path = str(tmp_path / "gt_dict.json")
    with open(gt_path, "w") as f:
        json.dump(inp["gt"], f)
    clf = make_clf(state, 512, p["num_nodes"])
    ops.launch_counters(reset=True)
    hr = eval_hit_rates_clf(emb, clf, gt_path, test_seq_len=p["test_seq_len"], k_probe=p["k_probe"])
    m, k = eval_map_clf(emb, clf, gt_path, k_probe=p["k_map_probe"], k_map=p["k_map"])
    cnt = clf_counts(ops)
    assert cnt["clf_pair_scores_n"] >= 2 and cnt["clf_pair_scores"] == 0
    np.testing.assert_array_equal(hr, z["eval/hit_rates"])
    for name, fname in (("hit_rates", "hit_rates_clf"), ("raw_score", "raw_score_clf"), ("test_ids", "test_ids_clf"),
                        ("map_score", "map_score")):
        got = np.load(os.path.join(emb, fname + ".npy"))
        assert got.dtype == z["eval/" + name].dtype and got.shape == z["eval/" + name].shape, name
        np.testing.assert_array_equal(got, z["eval/" + name])
    assert k == p["k_map"] and float(m) == float(z["eval/map_score"])
    pred = np.load(os.path.join(emb, "predictions.npy"), allow_pickle=True).item()
    assert pred == json.loads(bytes(z["eval/predictions"]).decode())


# ------------------------------------------------------------------------------------------------ bitwise invariance
@pytest.mark.parametrize("N", [128, 33])
def test_bitwise_invariance_and_run_to_run(N):
    C = 512
    clf = make_clf(rule_state(51 + N, C, 128), C, 128)
    q, c = nodes(52, 70, C, N), nodes(53, 6, C, N)
    with torch.no_grad():
        qp, kp = clf.project_queries(q), clf.project_candidates(c)
        # three groups, candidate lists with repeats, one group across the 64-segment chunk
        lists = [np.array([5, 0, 5, 3]), np.array([2]), np.array([1, 4, 4, 0, 5])]
        qs, qn = [0, 30, 3], [70, 2, 9]
        args = (qp, kp, N, qs, qn, np.concatenate(lists), np.cumsum([0] + [len(x) for x in lists[:-1]]), [len(x) for x in lists])
        big, off = clf.score_blocks(*args)
        again, _ = clf.score_blocks(*args)
        assert torch.equal(big, again)
        g0 = big[off[0]:off[0] + 70 * 4].view(70, 4)
        assert torch.equal(g0[:, 0], g0[:, 2])                      # a repeated candidate: bitwise the same score
        for (gi, qi, cj) in ((0, 0, 0), (0, 69, 3), (0, 64, 1), (1, 1, 0), (2, 8, 4), (2, 0, 2)):
            alone, _ = clf.score_blocks(qp, kp, N, [qs[gi] + qi], [1], [lists[gi][cj]], [0], [1])
            assert torch.equal(alone[0], big[off[gi] + qi * len(lists[gi]) + cj]), (gi, qi, cj)
        full = clf.pair_scores(q, c)
        one = clf.pair_scores(q[17:18].contiguous(), c[4:5].contiguous())
        assert torch.equal(one[0, 0], full[17, 4])
    assert float(full.std()) > 1e-3


# ------------------------------------------------------------------------------------------------ no read past the data
@pytest.mark.parametrize("N", [33, 97])
def test_no_read_past_the_projected_rows(N):
    """q and kp are the leading rows of larger NaN-filled buffers; the last candidate and the last query segment end at the last valid
    row. A read of any row at or beyond nq_seg N / nc_seg N would meet NaN (or, in a masked lane, would still be an access there)."""
    C, Sq, Sc = 512, 3, 2
    clf = make_clf(rule_state(61 + N, C, 128), C, 128)
    q, c = nodes(62, Sq, C, N), nodes(63, Sc, C, N)
    with torch.no_grad():
        qp, kp = clf.project_queries(q), clf.project_candidates(c)
        want, _ = clf.score_blocks(qp, kp, N, [0], [Sq], [0, 1], [0], [Sc])
        qbuf = torch.full((Sq * N + 160, C), float("nan"), device=DEV)
        kbuf = torch.full((Sc * N + 160, C + 512), float("nan"), device=DEV)
        qbuf[:Sq * N] = qp
        kbuf[:Sc * N] = kp
        qv, kv = qbuf[:Sq * N], kbuf[:Sc * N]
        assert qv.is_contiguous() and kv.is_contiguous() and qv.data_ptr() == qbuf.data_ptr()
        got, _ = clf.score_blocks(qv, kv, N, [0], [Sq], [0, 1], [0], [Sc])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ N <= 32 is untouched
def test_small_n_keeps_its_entries():
    _, ops, _ = _mods()
    C = 512
    clf = make_clf(rule_state(71, C, 128), C, 128)
    for N, new in ((32, False), (7, False), (64, True)):
        q, c = nodes(72 + N, 3, C, N), nodes(73 + N, 2, C, N)
        ops.launch_counters(reset=True)
        with torch.no_grad():
            clf.pair_scores(q, c)
        cnt = clf_counts(ops)
        old_n, new_n = (0, 1) if new else (1, 0)
        assert cnt["clf_pair_scores"] == old_n and cnt["clf_node_rows"] == 2 * old_n, (N, cnt)
        assert cnt["clf_pair_scores_n"] == new_n and cnt["clf_node_rows_n"] == 2 * new_n, (N, cnt)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    downstream, ops, _ = _mods()
    C = 512
    clf128 = make_clf(rule_state(81, C, 128), C, 128)
    clf64 = make_clf(rule_state(82, C, 64), C, 64)
    nopos = make_clf(rule_state(83, C, 128, pos_embed=False), C, 128, pos_embed=False)
    z = lambda S, N: torch.zeros(S, C, N, device=DEV)
    keep = torch.ones(2, 128, device=DEV)
    ops.launch_counters(reset=True)
    with torch.no_grad():
        bad = [
            (ValueError, lambda: clf128.pair_scores(z(2, 129), z(2, 129))),
            (ValueError, lambda: nopos.pair_scores(z(2, 129), z(2, 129))),
            (ValueError, lambda: nopos(z(2, 129), z(2, 129))),
            (ValueError, lambda: clf64.pair_scores(z(2, 100), z(2, 100))),
            (ValueError, lambda: clf128.pair_scores(z(2, 128), z(2, 64))),
            (ValueError, lambda: clf128(z(2, 128), z(2, 64))),
            (ValueError, lambda: ops.clf_node_rows(z(2, 129))),
            (ValueError, lambda: ops.clf_pair_scores(torch.zeros(258, C, device=DEV), torch.zeros(258, C + 512, device=DEV), 129,
                                                     torch.zeros(257, device=DEV), [0], [2], [0, 1], [0], [2])),
        ]
        for i, (exc, f) in enumerate(bad):
            with pytest.raises(exc):
                f()
            assert sum(ops.launch_counters().values()) == 0, i
    with pytest.raises(ValueError, match="training"):
        downstream.clf_train_scores(clf128, z(2, 64), z(2, 64), [0, 1], [0, 1], keep)
    assert sum(ops.launch_counters().values()) == 0


# ------------------------------------------------------------------------------------------------ the 256-mel encoder end to end
def test_256_mel_encoder_end_to_end(tmp_path):
    from synth import GRAFP_CFG, synth_randn, synth_state
    from neuralsampleid_amd import fpdb
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    cfg = dict(GRAFP_CFG, n_mels=256)
    model = SimCLR(cfg, GraphEncoder(cfg, in_channels=cfg["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV).eval()
    x = (synth_randn("clfnodes_x", 3, 256, cfg["n_frames"]) * 20 - 40).to(DEV)
    shapes = fpdb.build_node_matrices(model, [("a", x[:2]), ("b", x[2:])], str(tmp_path / "ref_nmatrix"), batch=2)
    assert shapes == {"a": (2, 512, 128), "b": (1, 512, 128)}
    nm = torch.from_numpy(np.concatenate([np.load(str(tmp_path / "ref_nmatrix" / f"{s}.npy")) for s in ("a", "b")])).to(DEV)
    assert nm.shape == (3, 512, 128) and nm.dtype == torch.float32 and bool(torch.isfinite(nm).all())
    state = rule_state(91, 512, 128)
    clf = make_clf(state, 512, 128)
    with torch.no_grad():
        s = clf.pair_scores(nm, nm)
    e = float((s.double() - fp64_scores(state, nm, nm)).abs().max())
    print(f"256-mel encoder end to end: |d| {e:.3g}, scores [{float(s.min()):.4f}, {float(s.max()):.4f}]")
    assert e < TOL
