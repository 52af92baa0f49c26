"""CPU: the oracle of the song-level votes (a dict-and-sorted restatement of eval.py:296-367 and eval_hr.py:85-156, pinned to the two
reference-made goldens), rejection_stats, and the refusals of SampleIndex that need no device. tests/test_identify_gpu.py compares
csrc/vote.hip with this oracle bit for bit."""
import json
import types

import numpy as np
import pytest
import torch


# ------------------------------------------------------------------------------------------------ the oracle
def _walk(I, k, s, L, song_of, n_dummy, excl):
    """walk positions j < L k of pair (s, L) that pass the candidate rules, with their song codes. song_of: one code per ref row; a
    negative code never votes (SampleIndex marks so the segments eval_hr.py skips: no node-matrix file, or a row past its end)"""
    for j in range(L * k):
        cid = int(I[s + j // k, j % k])
        if cid < 0 or cid < n_dummy or cid >= n_dummy + len(song_of):
            continue
        song = int(song_of[cid - n_dummy])
        if song < 0 or song == excl:
            continue
        yield j, song


def _ranked(hist):
    order = sorted(hist, key=hist.get, reverse=True)          # stable: ties in first-appearance (insertion) order
    return order, [hist[s] for s in order]


def vote_oracle(I, scores, starts, lens, song_of, n_dummy, exclude=None):
    """eval.py:296-367. Per pair: (song codes best first, their float64 totals). scores[p, j]: the score of walk position j"""
    k = I.shape[1]
    out = []
    for p, (s, L) in enumerate(zip(starts, lens)):
        hist = {}
        for j, song in _walk(I, k, int(s), int(L), song_of, n_dummy, -1 if exclude is None else int(exclude[p])):
            hist[song] = hist.get(song, 0.0) + float(scores[p, j])
        out.append(_ranked(hist))
    return out


def vote_oracle_clf(I, blocks, starts, lens, song_of, n_dummy, exclude=None, threshold=0.5):
    """eval_hr.py:85-156. blocks[p]: (>= L rows, >= L k columns) scores, column j = walk position j; the score of a candidate is the
    max over the first L rows, in the blocks' own precision, and is added when >= threshold"""
    k = I.shape[1]
    out = []
    for p, (s, L) in enumerate(zip(starts, lens)):
        hist = {}
        L = int(L)
        for j, song in _walk(I, k, int(s), L, song_of, n_dummy, -1 if exclude is None else int(exclude[p])):
            score = float(blocks[p][:L, j].max())
            if score >= threshold:
                hist[song] = hist.get(song, 0.0) + score
        out.append(_ranked(hist))
    return out


def hits(ranked, names, qids, gt, ti, si, n_tests, n_sl):
    """top-1/3/10 of every pair as the evaluations' raw_score (tests, 3 n_sl): the query id is in gt[song] for one of the first 1/3/10"""
    top = np.zeros((3, n_tests, n_sl), dtype=np.int64)
    for p, songs in enumerate(ranked):
        for m, lim in enumerate((1, 3, 10)):
            top[m, ti[p], si[p]] = int(any(qids[ti[p]] in gt.get(names[c], ()) for c in songs[:lim]))
    return np.concatenate([top[0], top[1], top[2]], axis=1)


def hit_rates(raw, lens, sl):
    valid = sl[None, :] <= np.asarray(lens)[:, None]
    n = sl.size
    with np.errstate(invalid="ignore"):
        return np.stack([100.0 * np.nanmean(np.where(valid, raw[:, m * n:(m + 1) * n], np.nan), axis=0) for m in range(3)], axis=0)


# ------------------------------------------------------------------------------------------------ the goldens as vote cases
def search_case():
    """search_l2.npz as a vote problem: everything SampleIndex.identify_pairs and the oracle need"""
    from make_search_golden import load_golden_inputs
    from neuralsampleid_amd.search import extract_test_ids, make_pairs, parse_seq_len
    z, inp = load_golden_inputs()
    params = json.loads(bytes(z["params"]).decode())
    return _case(z, inp, params, z["I"].astype(np.int64), extract_test_ids, make_pairs, parse_seq_len)


def _case(z, inp, params, I, extract_test_ids, make_pairs, parse_seq_len):
    sl = parse_seq_len(params["test_seq_len"])
    starts, lens = extract_test_ids(inp["query_lookup"])
    ti, si, ps, pl = make_pairs(starts, lens, sl)
    names = list(dict.fromkeys(inp["ref_lookup"]))            # codes in order of first appearance: SampleIndex's add order
    code = {n: c for c, n in enumerate(names)}
    qids = [inp["query_lookup"][int(s)].split("_")[0] for s in starts]
    return types.SimpleNamespace(z=z, inp=inp, params=params, I=I, k=int(I.shape[1]), sl=sl, starts=starts, lens=lens, ti=ti, si=si,
                                 ps=ps, pl=pl, names=names, qids=qids, n_dummy=inp["dummy"].shape[0],
                                 song_of=np.array([code[n] for n in inp["ref_lookup"]], dtype=np.int32),
                                 exclude=np.array([code.get(qids[t], -1) for t in ti], dtype=np.int64))


def rerank_case():
    """rerank_clf.npz as a vote problem; song_of_nodes is -1 where eval_hr.py skips a candidate for its node-matrix file"""
    from make_rerank_golden import load_golden_inputs
    from neuralsampleid_amd.rerank import ref_run_starts
    from neuralsampleid_amd.search import extract_test_ids, make_pairs, parse_seq_len
    z, inp, state = load_golden_inputs()
    params = json.loads(bytes(z["params"]).decode())
    c = _case(z, inp, params, z["I_hr"].astype(np.int64), extract_test_ids, make_pairs, parse_seq_len)
    seg = np.arange(len(inp["ref_lookup"])) - ref_run_starts(inp["ref_lookup"])
    rows = np.array([inp["ref_nm"][n].shape[0] if n in inp["ref_nm"] else 0 for n in inp["ref_lookup"]])
    c.song_of_nodes = np.where(seg < rows, c.song_of, -1).astype(np.int32)
    c.state = state
    return c


def walk_blocks(c, test_scores):
    """rerank's per-test (ascending candidate ids, S) as per-pair blocks whose column j is walk position j (NaN where the walk skips)"""
    blocks = []
    for p in range(c.ps.size):
        ids, S = test_scores[c.ti[p]]
        s, L = int(c.ps[p]), int(c.pl[p])
        col = {int(cid): n for n, cid in enumerate(np.asarray(ids).tolist())}
        B = np.full((L, L * c.k), np.nan, dtype=np.asarray(S).dtype)
        for j in range(L * c.k):
            cid = int(c.I[s + j // c.k, j % c.k])
            if cid in col:
                B[:, j] = S[:L, col[cid]]
        blocks.append(B)
    return blocks


def test_oracle_reproduces_the_search_golden():
    from make_search_golden import sequence_scores
    from neuralsampleid_amd.search import aggregate_hit_rates
    c = search_case()
    xb = np.concatenate([c.inp["dummy"], c.inp["ref"]])
    scores = sequence_scores(c.I, c.inp["query"], xb, c.starts, c.lens, c.sl, c.k)
    ranked = vote_oracle(c.I, scores, c.ps, c.pl, c.song_of, c.n_dummy, c.exclude)
    raw = hits([r[0] for r in ranked], c.names, c.qids, c.inp["gt"], c.ti, c.si, c.starts.size, c.sl.size)
    np.testing.assert_array_equal(raw, c.z["raw_score"])
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), c.z["hit_rates"])
    hr, raw_host, _ = aggregate_hit_rates(c.I, scores, c.inp["query_lookup"], c.inp["ref_lookup"], c.n_dummy, c.inp["gt"], c.sl)
    np.testing.assert_array_equal(raw, raw_host)
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), hr)
    assert raw.min() == 0 and raw.max() == 1


def test_oracle_reproduces_the_rerank_golden():
    from make_rerank_golden import fp64_classifier, host_scores
    from neuralsampleid_amd.rerank import vote_hit_rates_clf
    c = rerank_case()
    test_scores, ref_rows = host_scores(c.inp, c.I, fp64_classifier(c.state), c.params, False)
    ranked = vote_oracle_clf(c.I, walk_blocks(c, test_scores), c.ps, c.pl, c.song_of_nodes, c.n_dummy, c.exclude)
    raw = hits([r[0] for r in ranked], c.names, c.qids, c.inp["gt"], c.ti, c.si, c.starts.size, c.sl.size)
    np.testing.assert_array_equal(raw, c.z["raw_score"])
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), c.z["hit_rates"])
    hr, raw_host, _, skips = vote_hit_rates_clf(c.I, test_scores, c.inp["query_lookup"], c.inp["ref_lookup"], c.n_dummy, c.inp["gt"],
                                                ref_rows, c.sl)
    np.testing.assert_array_equal(raw, raw_host)
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), hr)
    assert skips[0] > 0 and skips[1] > 0 and (c.exclude >= 0).any() and (c.song_of_nodes < 0).any()


def test_oracle_ties_and_threshold_by_hand():
    I = np.array([[0, 1, 2, 3, 1, -1]], dtype=np.int64)
    song_of = np.array([5, 7, 5, 9], dtype=np.int32)
    sc = np.array([[0.25, 0.5, 0.25, 0.5, 0.125, 9.0]], dtype=np.float32)
    (songs, totals), = vote_oracle(I, sc, [0], [1], song_of, 0)
    assert songs == [7, 5, 9] and totals == [0.625, 0.5, 0.5]          # 5 and 9 tie: 5 appeared first
    (songs, totals), = vote_oracle(I, sc, [0], [1], song_of, 0, exclude=[7])
    assert songs == [5, 9] and totals == [0.5, 0.5]
    blk = np.array([[0.25, 0.5, 0.75, np.float32(0.5) - np.float32(2.0 ** -25), 0.125, 9.0]], dtype=np.float32)
    (songs, totals), = vote_oracle_clf(I, [blk], [0], [1], song_of, 0)
    assert songs == [5, 7] and totals == [0.75, 0.5]                    # song 5 enters at its second candidate


# ------------------------------------------------------------------------------------------------ rejection_stats
def test_rejection_stats_by_hand():
    from neuralsampleid_amd.identify import rejection_stats
    assert rejection_stats([0.9, 0.8, 0.7], [0.1, 0.2, 0.3, 0.4]) == (1.0, 4, 0)
    assert rejection_stats([0.1, 0.2], [0.8, 0.9]) == (0.0, 0, 2)
    a = [0.2, 0.6, 0.6, 0.9]
    assert rejection_stats(a, a)[0] == 0.5
    # ties: (0.5 | 0.5) counts a half, the three other pairs are ordered
    assert rejection_stats([0.5, 0.7], [0.5, 0.2])[0] == 3.5 / 4
    assert rejection_stats([1.0, 1.0], [1.0])[0] == 0.5
    # >= accepts
    auroc, rejects, accepts = rejection_stats([0.9], [0.5, float(np.nextafter(np.float64(0.5), 0.0)), 0.2, 0.75], threshold=0.5)
    assert (rejects, accepts) == (2, 2) and auroc == 1.0
    assert rejection_stats([0.9], [0.3, 0.3], threshold=0.3)[1:] == (0, 2)
    for real, dummy in (([], [0.1]), ([0.1], []), ([], [])):
        with pytest.raises(ValueError):
            rejection_stats(real, dummy)


def test_rejection_stats_against_sklearn_when_present():
    metrics = pytest.importorskip("sklearn.metrics")
    from neuralsampleid_amd.identify import rejection_stats
    rng = np.random.Generator(np.random.PCG64(3))
    real = np.round(rng.random(40) * 0.5 + 0.4, 2).tolist()             # rounded: many ties
    dummy = np.round(rng.random(55) * 0.6, 2).tolist()
    want = metrics.roc_auc_score([1] * len(real) + [0] * len(dummy), real + dummy)
    assert abs(rejection_stats(real, dummy)[0] - want) <= 1e-12


# ------------------------------------------------------------------------------------------------ refusals without a device
def _stub_model(d=128):
    return types.SimpleNamespace(projector=torch.nn.Sequential(torch.nn.Linear(8, d)), encoder=None, cfg={})


def test_sample_index_refusals_need_no_device():
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.identify import SampleIndex
    with pytest.raises(RuntimeError):
        SampleIndex(_stub_model(), device="cpu")
    idx = SampleIndex(_stub_model(128))
    assert idx.d == 128 and idx.n_ref == 0 and "a" not in idx
    with pytest.raises(RuntimeError):                       # CPU tensors
        idx.add_rows("a", torch.zeros(4, 128))
    with pytest.raises(RuntimeError):
        idx.add_dummy(torch.zeros(4, 128))
    with pytest.raises(RuntimeError):
        idx.identify(fp=torch.zeros(4, 128))
    with pytest.raises(RuntimeError):
        idx.add("a", specs=torch.zeros(2, 64, 32))
    for bad in (torch.zeros(4, 64), torch.zeros(128), torch.zeros(4, 128, dtype=torch.float64)):        # wrong d, rank, dtype
        with pytest.raises(ValueError):
            idx.add_rows("a", bad)
        with pytest.raises(ValueError):
            idx.identify(fp=bad)
    with pytest.raises(ValueError):
        SampleIndex(None).add_rows("a", torch.zeros(4, 100))             # a d the search kernels do not take
    with pytest.raises(TypeError):
        idx.add_rows("a", np.zeros((4, 128), np.float32))
    with pytest.raises(ValueError):
        idx.add("a")                                                      # neither specs nor wave
    with pytest.raises(RuntimeError):
        idx.add("a", wave=torch.zeros(8000))                              # no front end
    with pytest.raises(RuntimeError):                                     # rerank / node matrices without a classifier
        idx.identify(fp=torch.zeros(4, 128), rerank=True)
    with pytest.raises(RuntimeError):
        idx.add_rows("a", torch.zeros(4, 128), torch.zeros(4, 512, 32))
    with pytest.raises(RuntimeError):
        idx.match_score(torch.zeros(2, 512, 32), nodes=torch.zeros(2, 512, 32))
    with pytest.raises(KeyError):
        idx.code("nobody")
    clf = CrossAttentionClassifier(512, num_nodes=32)
    idx = SampleIndex(_stub_model(128), classifier=clf)
    for bad in (torch.zeros(4, 640, 32), torch.zeros(4, 512), torch.zeros(4, 512, 129)):                 # wrong C, rank, N
        with pytest.raises(ValueError):
            idx.add_rows("a", torch.zeros(4, 128), bad)
    with pytest.raises(RuntimeError):
        idx.match_score(torch.zeros(2, 512, 32), nodes=torch.zeros(2, 512, 32))                          # CPU tensors
    with pytest.raises(ValueError):
        idx.match_score(torch.zeros(2, 512, 32))
    assert idx.n_ref == 0 and idx.names == []


def test_vote_bindings_and_counters():
    from neuralsampleid_amd import _lib, ops
    assert _lib.SIGNATURES["nsid_song_vote"] == "pipippipiipippps"
    assert _lib.SIGNATURES["nsid_song_vote_clf"] == "pipppppipiipfippps"
    assert _lib.SIGNATURES["nsid_vote_candidates"] == "pliips"
    assert {"song_vote", "song_vote_clf", "vote_candidates"} <= set(ops.launch_counters())
    assert ops.VOTE_MAX_CAND == 4096 and ops.VOTE_MAX_TOP == 32
    # CPU tensors are refused by the ops as well
    I = torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.song_vote(I, torch.zeros(1, 20), [0], [4], torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError):
        ops.vote_candidates(I, 0, 3)
