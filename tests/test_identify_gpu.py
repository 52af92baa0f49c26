"""GPU: the song-level votes of csrc/vote.hip against the dict-and-sorted oracle of tests/test_identify_cpu.py (song codes, n_songs
and the fp64 totals bit for bit: both sides add the same fp32 values in fp64 in the same order), SampleIndex on the two
reference-made goldens and end to end on the synthetic 't' encoder, its invariants and its refusals."""
import json
import math

import numpy as np
import pytest
import torch

from test_identify_cpu import hit_rates, hits, rerank_case, search_case, vote_oracle, vote_oracle_clf, walk_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BELOW_HALF = float(np.float32(0.5) - np.float32(2.0 ** -25))          # the fp32 number just below 0.5


@pytest.fixture(autouse=True)
def _fp32_switches():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def assert_votes_equal(got, ranked, top):
    """device (songs, totals, n_songs) against the oracle's per-pair (codes, totals): exact, the totals as bit patterns"""
    songs, totals, n = (t.cpu().numpy() for t in got)
    P = len(ranked)
    assert songs.shape == (P, top) and totals.shape == (P, top) and n.shape == (P,)
    assert songs.dtype == np.int32 and totals.dtype == np.float64 and n.dtype == np.int32
    want_s = np.full((P, top), -1, dtype=np.int32)
    want_t = np.zeros((P, top), dtype=np.float64)
    for p, (codes, tot) in enumerate(ranked):
        m = min(top, len(codes))
        want_s[p, :m] = codes[:m]
        want_t[p, :m] = tot[:m]
    np.testing.assert_array_equal(n, [len(r[0]) for r in ranked])
    np.testing.assert_array_equal(songs, want_s)
    np.testing.assert_array_equal(totals.view(np.int64), want_t.view(np.int64))


# ------------------------------------------------------------------------------------------------ 1. the kernels against the oracle
# every L k of {1, 63, 64, 65, 380, 4096} at the k of {1, 5, 20, 64} that divide it
PAIRS_BY_K = {1: [1, 63, 64, 65, 380, 4096], 5: [13, 76], 20: [19], 64: [1, 64]}
VALUES = np.array([0.25, 0.5, -0.25, 1.0, 0.125, -1.0, 0.75, 3.0], dtype=np.float32)      # few dyadic values: exact ties abound


def random_problem(seed, k, lens, n_songs, n_ref=97, n_dummy=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, dtype=np.int64)
    rows = int(lens.max()) + 3
    starts = np.array([int(rng.integers(0, rows - L + 1)) for L in lens], dtype=np.int64)
    # ids: -1, dummies, ref rows (repeats likely: few rows for the long walks), and ids past the end
    I = rng.integers(-1, n_dummy + n_ref + 4, size=(rows, k)).astype(np.int64)
    song_of = rng.integers(0, n_songs, size=n_ref).astype(np.int32)
    exclude = rng.integers(-1, n_songs, size=lens.size).astype(np.int64)
    scores = VALUES[rng.integers(0, VALUES.size, size=(lens.size, int(lens.max()) * k))]
    return I, scores, starts, lens, song_of, n_dummy, exclude


@pytest.mark.parametrize("n_songs,top", [(1, 10), (3, 10), (60, 10), (60, 32), (3, 1)])
@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_song_vote_matches_oracle(k, n_songs, top):
    from neuralsampleid_amd import ops
    I, scores, starts, lens, song_of, n_dummy, exclude = random_problem(1000 + 7 * k + n_songs, k, PAIRS_BY_K[k], n_songs)
    ranked = vote_oracle(I, scores, starts, lens, song_of, n_dummy, exclude)
    if n_songs == 60:
        assert max(len(r[0]) for r in ranked) > top or top == 32
    ops.launch_counters(reset=True)
    got = ops.song_vote(_dev(I), _dev(scores), starts, lens, _dev(song_of), n_dummy, exclude, top)
    assert ops.launch_counters()["song_vote"] == 1
    assert_votes_equal(got, ranked, top)
    # without an exclusion list
    assert_votes_equal(ops.song_vote(_dev(I), _dev(scores), starts, lens, _dev(song_of), n_dummy, None, top),
                       vote_oracle(I, scores, starts, lens, song_of, n_dummy), top)


def clf_problem(seed, k, lens, n_songs):
    """pairs over shared starts: the pairs of one start read one block at the longest length (a shorter walk is a prefix)"""
    I, _, _, lens, song_of, n_dummy, exclude = random_problem(seed, k, lens, n_songs)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    starts = np.zeros(lens.size, dtype=np.int64)
    starts[1::2] = 2 if I.shape[0] - int(lens.max()) >= 2 else 0
    vals = np.array([0.5, BELOW_HALF, 0.75, 0.25, 0.5 + 2.0 ** -24, 0.9375, 0.0], dtype=np.float32)
    blocks, s_off, s_ld, flat, pos = {}, [], [], [], 0
    for s in np.unique(starts).tolist():
        Lmax = int(lens[starts == s].max())
        B = vals[rng.integers(0, vals.size, size=(Lmax, Lmax * k + 3))]          # rows 3 floats longer than the walk
        blocks[s] = (pos, B)
        flat.append(B.reshape(-1))
        pos += B.size
    per_pair = []
    for s in starts.tolist():
        off, B = blocks[s]
        s_off.append(off)
        s_ld.append(B.shape[1])
        per_pair.append(B)
    return I, np.concatenate(flat), per_pair, np.array(s_off), np.array(s_ld), starts, lens, song_of, n_dummy, exclude


@pytest.mark.parametrize("n_songs,top", [(1, 10), (3, 10), (60, 10)])
@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_song_vote_clf_matches_oracle(k, n_songs, top):
    from neuralsampleid_amd import ops
    lens = [L for L in PAIRS_BY_K[k] if L * L * k <= 1 << 20] or [1]          # a block is L x L k scores: the long k = 1 walks below
    I, flat, blocks, s_off, s_ld, starts, lens, song_of, n_dummy, exclude = clf_problem(2000 + 7 * k + n_songs, k, lens, n_songs)
    ranked = vote_oracle_clf(I, blocks, starts, lens, song_of, n_dummy, exclude)
    ops.launch_counters(reset=True)
    got = ops.song_vote_clf(_dev(I), _dev(flat), s_off, s_ld, starts, lens, _dev(song_of), n_dummy, exclude, 0.5, top)
    assert ops.launch_counters()["song_vote_clf"] == 1
    assert_votes_equal(got, ranked, top)


def test_song_vote_clf_longest_walk():
    """L k = 4096 at k = 64 and at k = 1 with one-row blocks stretched by a zero row stride (every row the same: the max is the row)"""
    from neuralsampleid_amd import ops
    for k, L in ((64, 64), (1, 4096)):
        I, _, _, lens, song_of, n_dummy, exclude = random_problem(3000 + k, k, [L], 60)
        rng = np.random.Generator(np.random.PCG64(5 + k))
        row = np.array([0.5, BELOW_HALF, 0.75, 0.625], dtype=np.float32)[rng.integers(0, 4, size=(1, L * k))]
        ranked = vote_oracle_clf(I, [np.repeat(row, L, 0)], [0], [L], song_of, n_dummy, exclude[:1])
        got = ops.song_vote_clf(_dev(I), _dev(row.reshape(-1)), [0], [0], [0], [L], _dev(song_of), n_dummy, exclude[:1], 0.5, 10)
        assert_votes_equal(got, ranked, 10)


def test_votes_by_hand():
    """forced exact ties of two and three songs first seen in either order, an excluded song, a pair with nothing left, and the
    threshold's edge: exactly 0.5 enters, the number below does not, a song enters at its first PASSING candidate"""
    from neuralsampleid_amd import ops
    song_of = _dev(np.array([0, 1, 2, 0, 1, 2, 3], dtype=np.int32))
    n_dummy = 2
    r = lambda *ids: [i + n_dummy for i in ids]
    I = np.array([r(0, 1, 3, 2, 4, 5),            # songs 0 1 0 2 1 2
                  r(2, 1, 5, 0, 4, 3),            # songs 2 1 2 0 1 0: the same sums, first seen in the other order
                  r(6, 0, 1, 6, 3, 4),            # songs 3 0 1 3 0 1
                  [-1, 0, 1, 99, -1, 1]], dtype=np.int64)          # none, dummies, past the end
    sc = np.array([[0.5, 0.25, 0.25, 0.5, 0.5, 0.25]] * 4, dtype=np.float32)
    sc[2] = [1.0, 0.25, 0.5, 1.0, 0.5, 0.25]     # song 3: 2.0, songs 0 and 1 tie at 0.75
    starts, lens = [0, 1, 2, 3, 2], [1, 1, 1, 1, 1]
    scores = sc[[0, 1, 2, 3, 2]]
    got = ops.song_vote(_dev(I), _dev(scores), starts, lens, song_of, n_dummy, [-1, -1, -1, -1, 3], 4)
    songs, totals, n = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(songs, [[0, 1, 2, -1], [2, 1, 0, -1], [3, 0, 1, -1], [-1, -1, -1, -1], [0, 1, -1, -1]])
    np.testing.assert_array_equal(totals, [[0.75, 0.75, 0.75, 0], [0.75, 0.75, 0.75, 0], [2.0, 0.75, 0.75, 0], [0, 0, 0, 0],
                                           [0.75, 0.75, 0, 0]])
    np.testing.assert_array_equal(n, [3, 3, 3, 0, 2])
    assert_votes_equal(got, vote_oracle(I, scores, starts, lens, song_of.cpu().numpy(), n_dummy, [-1, -1, -1, -1, 3]), 4)
    # classifier rule on row 0 (songs 0 1 0 2 1 2), two query rows: the max over the rows decides
    S = np.array([[BELOW_HALF, 0.5, 0.25, BELOW_HALF, 0.25, 0.75],
                  [0.25, 0.125, 0.75, 0.25, BELOW_HALF, 0.5]], dtype=np.float32)
    I2 = np.concatenate([I[:1], I[:1]])           # L = 2 walks both rows: 12 candidates, block columns 0..11
    S2 = np.concatenate([S, S[:, ::-1]], axis=1)
    got = ops.song_vote_clf(_dev(I2), _dev(S2.reshape(-1)), [0, 0], [12, 12], [0, 0], [1, 2], song_of, n_dummy, None, 0.5, 3)
    ranked = vote_oracle_clf(I2, [S2, S2], [0, 0], [1, 2], song_of.cpu().numpy(), n_dummy)
    assert_votes_equal(got, ranked, 3)
    songs = got[0].cpu().numpy()
    # L = 1: song 0's candidates both fail (below 0.5), song 1 enters at exactly 0.5 ahead of song 2 (0.75) in appearance, behind in sum
    np.testing.assert_array_equal(songs[0], [2, 1, -1])
    np.testing.assert_array_equal(got[1].cpu().numpy()[0], [0.75, 0.5, 0.0])


def test_vote_candidates():
    from neuralsampleid_amd import ops
    I = np.array([[-1, 0, 4, 5], [9, 10, 11, 2 ** 40]], dtype=np.int64)
    ops.launch_counters(reset=True)
    out = ops.vote_candidates(_dev(I), 5, 5)
    assert ops.launch_counters()["vote_candidates"] == 1 and out.dtype == torch.int32 and out.shape == (2, 4)
    np.testing.assert_array_equal(out.cpu().numpy(), [[0, 0, 0, 0], [4, 0, 0, 0]])
    big = np.random.Generator(np.random.PCG64(1)).integers(-1, 3000, size=(777, 13)).astype(np.int64)
    want = np.where((big >= 100) & (big < 2100), big - 100, 0).astype(np.int32)
    np.testing.assert_array_equal(ops.vote_candidates(_dev(big), 100, 2000).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 2. the reference-made goldens
def _runs(lookup):
    from neuralsampleid_amd.search import extract_test_ids
    starts, lens = extract_test_ids(lookup)
    return [(lookup[int(s)], int(s), int(n)) for s, n in zip(starts, lens)]


def _exclude_names(c, idx):
    return [c.qids[t] if c.qids[t] in idx else None for t in c.ti]


def test_identify_pairs_reproduces_the_search_golden():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    c = search_case()
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(c.inp["dummy"]))
    ref = _dev(c.inp["ref"])
    for name, s, n in _runs(c.inp["ref_lookup"]):
        idx.add_rows(name, ref[s:s + n])
    assert idx.names == c.names and idx.n_dummy == c.n_dummy and idx.n_ref == ref.shape[0] and idx.d == 128
    q = _dev(c.inp["query"])
    ops.launch_counters(reset=True)
    pv = idx.identify_pairs(q, c.ps, c.pl, k_probe=c.k, top=10, exclude=_exclude_names(c, idx))
    cnt = ops.launch_counters()
    assert cnt["song_vote"] == 1 and cnt["seq_scores"] == 1 and cnt["song_vote_clf"] == 0
    res = pv.results()
    code = {n: i for i, n in enumerate(idx.names)}
    raw = hits([[code[s] for s in r.songs] for r in res], c.names, c.qids, c.inp["gt"], c.ti, c.si, c.starts.size, c.sl.size)
    np.testing.assert_array_equal(raw, c.z["raw_score"])
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), c.z["hit_rates"])
    # and the oracle on the device's own I and sequence scores, exactly
    _, I = idx._index.search(q, c.k)
    np.testing.assert_array_equal(I.cpu().numpy(), c.I)
    scores = ops.seq_scores(q, idx._index.xb, I, c.ps, c.pl, int(c.pl.max()) * c.k).cpu().numpy()
    assert_votes_equal((pv.codes, pv.totals, pv.n_songs), vote_oracle(c.I, scores, c.ps, c.pl, c.song_of, c.n_dummy, c.exclude), 10)


def test_identify_pairs_rerank_reproduces_the_rerank_golden(tmp_path):
    from make_rerank_golden import write_inputs
    from neuralsampleid_amd import ops, rerank
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.identify import SampleIndex
    c = rerank_case()
    clf = CrossAttentionClassifier(in_dim=512, num_nodes=c.params["num_nodes"])
    clf.load_state_dict(c.state, strict=True)
    clf = clf.to(DEV).eval()
    idx = SampleIndex(None, classifier=clf, device=DEV)
    idx.add_dummy(_dev(c.inp["dummy"]))
    ref = _dev(c.inp["ref"])
    for name, s, n in _runs(c.inp["ref_lookup"]):
        nm = c.inp["ref_nm"].get(name)                       # one song has no file, one has fewer rows than segments
        idx.add_rows(name, ref[s:s + n], None if nm is None else _dev(nm))
    np.testing.assert_array_equal(idx._song_of_nodes[: idx.n_ref].cpu().numpy(), c.song_of_nodes)
    np.testing.assert_array_equal(idx._song_of[: idx.n_ref].cpu().numpy(), c.song_of)
    assert idx.kp_bytes_per_segment == 4 * 32 * (512 + 512)
    q = _dev(c.inp["query"])
    qnodes = _dev(np.concatenate([c.inp["query_nm"][qid] for qid in dict.fromkeys(c.qids)]))
    assert qnodes.shape[0] == q.shape[0]
    ops.launch_counters(reset=True)
    pv = idx.identify_pairs(q, c.ps, c.pl, k_probe=c.k, top=10, exclude=_exclude_names(c, idx), rerank=True, nodes=qnodes)
    cnt = ops.launch_counters()
    assert cnt["song_vote_clf"] == 1 and cnt["vote_candidates"] == 1 and cnt["clf_pair_scores"] == 1 and cnt["song_vote"] == 0
    res = pv.results()
    code = {n: i for i, n in enumerate(idx.names)}
    raw = hits([[code[s] for s in r.songs] for r in res], c.names, c.qids, c.inp["gt"], c.ti, c.si, c.starts.size, c.sl.size)
    np.testing.assert_array_equal(raw, c.z["raw_score"])
    np.testing.assert_array_equal(hit_rates(raw, c.lens, c.sl), c.z["hit_rates"])
    # the device-list score blocks: bit for bit what rerank.score_tests gives for the same pairs
    _, I = idx._index.search(q, c.k)
    np.testing.assert_array_equal(I.cpu().numpy(), c.I)
    emb = str(tmp_path / "emb")
    write_inputs(c.inp, emb)
    ref_dir = emb + "/ref_nmatrix"
    walk = rerank._Walk(c.inp["ref_lookup"], c.n_dummy, rerank._ref_rows(ref_dir, sorted(set(c.inp["ref_lookup"]))))
    tests = []
    for t, (s0, L) in enumerate(zip(c.starts.tolist(), c.lens.tolist())):
        msl = int(c.sl[c.sl <= L].max()) if (c.sl <= L).any() else 0
        tests.append((c.qids[t], msl, rerank.candidate_ids(c.I[s0:s0 + msl], c.qids[t], walk) if msl else np.zeros(0, np.int64)))
    host = walk_blocks(c, rerank.score_tests(clf, tests, c.inp["query_nm"], ref_dir, c.inp["ref_lookup"], c.n_dummy, DEV))
    flat = pv.scores.cpu().numpy()
    dev_blocks, compared = [], 0
    for p in range(c.ps.size):
        L, ld = int(c.pl[p]), int(pv.s_ld[p])
        B = flat[int(pv.s_off[p]): int(pv.s_off[p]) + (L - 1) * ld + L * c.k]
        B = np.stack([B[i * ld: i * ld + L * c.k] for i in range(L)])
        dev_blocks.append(B)
        keep = ~np.isnan(host[p])
        compared += int(keep.sum())
        np.testing.assert_array_equal(B[keep].view(np.int32), host[p][keep].view(np.int32))
    assert compared > 200
    assert_votes_equal((pv.codes, pv.totals, pv.n_songs),
                       vote_oracle_clf(c.I, dev_blocks, c.ps, c.pl, c.song_of_nodes, c.n_dummy, c.exclude), 10)


# ------------------------------------------------------------------------------------------------ 3. end to end on the 't' encoder
# chosen on the fp64 module alone, among rule_state seeds 20..43: the encoder's node matrices have a standard deviation of about 15, which
# saturates most random classifiers to 0 or 1; this one scores own songs 0.46 / 0.97 / 0.82 and the noise nodes 0.09 / 0.18 / 0.34
CLF_SEED = 30


def rule_state(seed, num_nodes=32):
    rng = np.random.Generator(np.random.PCG64(seed))
    C, hid = 512, 128
    n = lambda *s, scale: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32))
    return {"attn.in_proj_weight": n(3 * C, C, scale=C ** -0.5), "attn.in_proj_bias": n(3 * C, scale=0.1),
            "attn.out_proj.weight": n(C, C, scale=C ** -0.5), "attn.out_proj.bias": n(C, scale=0.1),
            "fc.0.weight": n(hid, C, scale=2.0 * C ** -0.5), "fc.0.bias": n(hid, scale=0.1),
            "fc.3.weight": n(1, hid, scale=2.0 * hid ** -0.5), "fc.3.bias": n(1, scale=0.1),
            "positional_embedding": n(1, num_nodes, C, scale=0.5)}


class Ref64(torch.nn.Module):
    """fp64 eval-mode forward of the reference module (downstream.py:30-78)"""

    def __init__(self, state):
        super().__init__()
        nn = torch.nn
        self.register_buffer("positional_embedding", torch.zeros(state["positional_embedding"].shape))
        self.attn = nn.MultiheadAttention(embed_dim=512, num_heads=4, batch_first=True)
        self.fc = nn.Sequential(nn.Linear(512, 128), nn.ReLU(), nn.Dropout(p=0.3), nn.Linear(128, 1), nn.Sigmoid())
        self.load_state_dict(state, strict=True)
        self.double().eval()

    @torch.no_grad()
    def forward(self, x_i, x_j):
        x_i, x_j = x_i.permute(0, 2, 1), x_j.permute(0, 2, 1)
        pos = self.positional_embedding[:, :x_i.shape[1], :]
        a, _ = self.attn(x_i + pos, x_j + pos, x_j + pos)
        return self.fc(a.mean(dim=1))

    def match_score(self, nodes_q, nodes_r):
        """ablation.py:84-97"""
        q, r = nodes_q.double().cpu(), nodes_r.double().cpu()
        return float(np.mean([float(self(x[None].repeat(r.shape[0], 1, 1), r).max()) for x in q]))


@pytest.fixture(scope="module")
def synth_index():
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.identify import SampleIndex
    from neuralsampleid_amd.simclr.simclr import SimCLR
    from synth import GRAFP_CFG, synth_clips, synth_state
    torch.manual_seed(0)
    model = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict(), ""))
    model = model.to(DEV).eval()
    state = rule_state(CLF_SEED)
    clf = CrossAttentionClassifier(512, num_nodes=32)
    clf.load_state_dict(state, strict=True)
    clf = clf.to(DEV).eval()
    x, _ = synth_clips(24)
    x = x.to(DEV)
    idx = SampleIndex(model, classifier=clf, device=DEV)
    for i in range(6):
        assert idx.add(f"song{i}", specs=x[4 * i:4 * i + 4]) == 4
    return idx, model, clf, x, state


def test_add_stores_what_the_extractors_give(synth_index):
    from neuralsampleid_amd.fingerprint import extract_fingerprints
    from neuralsampleid_amd.fpdb import extract_node_matrices
    idx, model, clf, x, _ = synth_index
    assert idx.n_ref == 24 and idx.names == [f"song{i}" for i in range(6)] and idx.N == 32 and idx.d == 128
    np.testing.assert_array_equal(idx._song_of[:24].cpu().numpy(), np.repeat(np.arange(6), 4))
    for i in range(6):
        specs = x[4 * i:4 * i + 4]
        assert torch.equal(idx.fingerprints[4 * i:4 * i + 4], extract_fingerprints(model, specs))
        nodes = extract_node_matrices(model, specs)
        fp, enc_nodes = idx._encode(specs, True)
        assert torch.equal(enc_nodes, nodes) and torch.equal(fp, idx.fingerprints[4 * i:4 * i + 4])
        with torch.no_grad():
            assert torch.equal(idx._kp[4 * i * 32:(4 * i + 4) * 32], clf.project_candidates(nodes))
    assert not model.training


def test_queries_cut_from_a_song_are_identified(synth_index):
    idx, model, clf, x, _ = synth_index
    for i in (1, 3, 4):
        # k_probe = 1: each query segment votes for the song of its nearest row only (test_end_to_end_extraction_search)
        r = idx.identify(specs=x[4 * i + 1:4 * i + 3], k_probe=1, top=3)
        assert r.songs[0] == f"song{i}" and r.n_songs >= 1 and r.totals.dtype == np.float64 and len(r.totals) == len(r.songs), r
        assert r.totals[0] > 1.9                                   # two segments, each the unit dot of a row with itself
        r2 = idx.identify(specs=x[4 * i + 1:4 * i + 3], k_probe=1, top=3, exclude=f"song{i}")
        assert f"song{i}" not in r2.songs
        rr = idx.identify(specs=x[4 * i + 1:4 * i + 3], k_probe=3, top=5, rerank=True)
        assert rr.n_songs >= len(rr.songs) and all(t >= 0.5 for t in rr.totals)
    with pytest.raises(KeyError):
        idx.identify(specs=x[:2], exclude="nobody")


def _tone(seconds, f0, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * 16000)
    t = torch.arange(n) / 16000.0
    w = 0.3 * torch.sin(2 * math.pi * f0 * t) + 0.1 * torch.sin(2 * math.pi * 2.7 * f0 * t * (1 + 0.05 * t))
    return (w + 0.05 * torch.randn(n, generator=g)).float()


def test_waveforms_through_the_front_end(synth_index):
    from neuralsampleid_amd.fingerprint import fingerprints_from_waveform
    from neuralsampleid_amd.frontend import LogMelFrontEnd
    from neuralsampleid_amd.identify import SampleIndex
    _, model, _, _, _ = synth_index
    cfg = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875}
    front = LogMelFrontEnd(cfg, DEV)
    idx = SampleIndex(model, front=front, device=DEV)
    waves = [_tone(5.6, f0, s).to(DEV) for s, f0 in enumerate((220.0, 523.0, 1310.0))]
    for i, w in enumerate(waves):
        n = idx.add(f"tone{i}", wave=w)
        assert n == front(w).shape[0] >= 2
    assert torch.equal(idx.fingerprints[: n], fingerprints_from_waveform(model, front, waves[0]))
    r = idx.identify(wave=waves[1], k_probe=1, top=2)
    assert r.songs[0] == "tone1", r
    with pytest.raises(ValueError):
        idx.identify(wave=torch.zeros(20000, device=DEV))            # shorter than one segment
    with pytest.raises(RuntimeError):
        idx.identify(specs=front(waves[0]), rerank=True)             # no classifier


def test_match_score_prefers_the_own_song(synth_index):
    """ablation.py's rejection score: a query cut from a song against that song, and against noise nodes. The fp64 module alone
    shows the gap with margin; the device scores then agree with it to fp32 accuracy and keep the order."""
    from neuralsampleid_amd.fpdb import extract_node_matrices
    from neuralsampleid_amd.identify import rejection_stats
    idx, model, clf, x, state = synth_index
    ref = Ref64(state)
    real, dummy = [], []
    for i in (1, 3, 4):
        nq = extract_node_matrices(model, x[4 * i + 1:4 * i + 3])
        own = extract_node_matrices(model, x[4 * i:4 * i + 4])
        g = torch.Generator().manual_seed(i)
        noise = torch.randn(1, 512, 32, generator=g).to(DEV)        # the reference's torch.randn_like(nm_q): one segment
        want_own, want_noise = ref.match_score(nq, own), ref.match_score(nq, noise)
        print(f"song{i}: fp64 own {want_own:.6f} noise {want_noise:.6f}")
        assert want_own - want_noise > 0.3, (want_own, want_noise)
        got_own, got_noise = idx.match_score(nq, f"song{i}"), idx.match_score(nq, nodes=noise)
        print(f"song{i}: device own {got_own:.6f} ({got_own - want_own:+.2e}) noise {got_noise:.6f} ({got_noise - want_noise:+.2e})")
        # fp32 against fp64: the nodes' standard deviation of 15 puts the attention logits at the order of 1e2..1e3, so their fp32 rounding
        # (6e-8 relative per operation over 512-long dots) is of the order of 1e-4 before the softmax and the two linears amplify it;
        # 5e-3 on the score bounds that with room and is 60 times below the gap asserted above
        assert abs(got_own - want_own) < 5e-3 and abs(got_noise - want_noise) < 5e-3, (got_own, want_own, got_noise, want_noise)
        assert got_own > got_noise
        real.append(got_own)
        dummy.append(got_noise)
    assert rejection_stats(real, dummy)[0] == 1.0
    with pytest.raises(KeyError):
        idx.match_score(nq, "nobody")


# ------------------------------------------------------------------------------------------------ 4. invariants
def test_invariants_runs_batches_and_pairs():
    from neuralsampleid_amd import ops
    I, scores, starts, lens, song_of, n_dummy, exclude = random_problem(77, 5, [1 + (i * 7) % 60 for i in range(50)], 9)
    Id, sd, so = _dev(I), _dev(scores), _dev(song_of)
    a = ops.song_vote(Id, sd, starts, lens, so, n_dummy, exclude, 10)
    b = ops.song_vote(Id, sd, starts, lens, so, n_dummy, exclude, 10)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for p in (0, 17, 49):
        one = ops.song_vote(Id, sd[p:p + 1], starts[p:p + 1], lens[p:p + 1], so, n_dummy, exclude[p:p + 1], 10)
        assert torch.equal(one[0][0], a[0][p]) and torch.equal(one[1][0].view(torch.int64), a[1][p].view(torch.int64))
        assert int(one[2][0]) == int(a[2][p])


def test_invariants_of_the_index(synth_index):
    from neuralsampleid_amd.identify import SampleIndex
    idx, model, clf, x, _ = synth_index
    fp = idx.fingerprints[4:16].clone()
    pv = idx.identify_pairs(fp, [0, 0, 3], [5, 12, 2], k_probe=4, top=6)
    again = idx.identify_pairs(fp, [0, 0, 3], [5, 12, 2], k_probe=4, top=6)
    assert torch.equal(pv.codes, again.codes) and torch.equal(pv.totals.view(torch.int64), again.totals.view(torch.int64))
    r = idx.identify(fp=fp[:5], k_probe=4, top=6)
    first = pv.results()[0]
    assert r.songs == first.songs and r.n_songs == first.n_songs and len(r.songs) >= 1
    np.testing.assert_array_equal(r.totals.view(np.int64), first.totals.view(np.int64))
    # growth by doubling keeps earlier results: the same songs one by one into a fresh index (capacities 4, 8, 16, 32 rows)
    grown = SampleIndex(model, classifier=clf, device=DEV)
    firsts = []
    for i in range(6):
        grown.add_rows(f"song{i}", idx.fingerprints[4 * i:4 * i + 4].clone())
        firsts.append(grown.identify(fp=fp[:2], k_probe=1, top=1))
    assert grown._song_of.shape[0] == 32 and grown.n_ref == 24
    assert all(f.songs == ["song1"] and f.totals[0] == firsts[1].totals[0] for f in firsts[1:])
    g = grown.identify_pairs(fp, [0, 0, 3], [5, 12, 2], k_probe=4, top=6)
    assert torch.equal(g.codes, pv.codes) and torch.equal(g.totals.view(torch.int64), pv.totals.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 5. refusals launch nothing
def test_refusals_launch_nothing(synth_index):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import lib
    from neuralsampleid_amd.identify import SampleIndex
    idx, model, clf, x, _ = synth_index
    I = torch.zeros((4100, 1), device=DEV, dtype=torch.int64)
    I64 = torch.zeros((80, 64), device=DEV, dtype=torch.int64)
    sc = torch.zeros((1, 4096), device=DEV)
    so = torch.zeros((8,), device=DEV, dtype=torch.int32)
    fp = idx.fingerprints[:8].clone()
    torch.cuda.synchronize()
    ops.launch_counters(reset=True)
    for fn in (lambda: ops.song_vote(I, sc, [0], [4097], so, 0), lambda: ops.song_vote(I64, sc, [0], [65], so, 0),
               lambda: ops.song_vote(I, sc, [0], [10], so, 0, None, 33), lambda: ops.song_vote(I, sc, [0], [10], so, 0, None, 0),
               lambda: ops.song_vote(I, sc, [0], [0], so, 0), lambda: ops.song_vote(I, sc, [4095], [10], so, 0),
               lambda: ops.song_vote(I, sc[:, :5], [0], [10], so, 0), lambda: ops.song_vote(I, sc, [0], [10], so, 0, [1, 2]),
               lambda: ops.song_vote(torch.zeros((4, 65), device=DEV, dtype=torch.int64), sc, [0], [1], so, 0),
               lambda: ops.song_vote_clf(I, sc.reshape(-1), [0], [1], [0], [4097], so, 0),
               lambda: ops.song_vote_clf(I, sc.reshape(-1), [0], [4096], [0], [2], so, 0),           # the block leaves S
               lambda: ops.song_vote_clf(I, sc.reshape(-1), [0], [1], [0], [10], so, 0, None, 0.5, 33),
               lambda: ops.vote_candidates(I, -1, 5),
               lambda: idx.identify(fp=fp, top=33), lambda: idx.identify(fp=fp, k_probe=65),
               lambda: idx.identify_pairs(idx.fingerprints[:1].expand(70, 128).contiguous(), [0], [70], k_probe=64),      # L k = 4480
               lambda: idx.identify(fp=torch.zeros(4, 64, device=DEV)), lambda: idx.identify_pairs(fp, [0], [9]),
               lambda: idx.identify(fp=fp, rerank=True),                                              # no node matrices given
               lambda: idx.identify(fp=fp, rerank=True, nodes=torch.zeros(8, 512, 16, device=DEV)),   # another N
               lambda: idx.add_rows("song0", fp), lambda: idx.add_rows("new", fp, torch.zeros(8, 640, 32, device=DEV))):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: idx.add_dummy(fp), lambda: SampleIndex(model, device=DEV).identify(fp=fp, rerank=True),
               lambda: SampleIndex(model, device=DEV).identify(fp=fp),                                # an empty index
               lambda: ops.song_vote(I.int(), sc, [0], [10], so, 0), lambda: ops.song_vote(I, sc, [0], [10], so.long(), 0)):
        with pytest.raises(RuntimeError):
            fn()
    assert idx.n_ref == 24 and "new" not in idx
    cnt = ops.launch_counters()
    assert sum(cnt.values()) == 0, {k: v for k, v in cnt.items() if v}
    # the C entries refuse k = 65, top = 33 and L k = 4097 (song_vote's lds bounds every pair's L k) before any launch
    out_s = torch.empty((1, 33), device=DEV, dtype=torch.int32)
    out_t = torch.empty((1, 33), device=DEV, dtype=torch.float64)
    out_n = torch.empty((1,), device=DEV, dtype=torch.int32)
    one = torch.ones((1,), device=DEV, dtype=torch.int32)
    zero = torch.zeros((1,), device=DEV, dtype=torch.int32)
    off = torch.zeros((1,), device=DEV, dtype=torch.int64)
    big = torch.zeros((1, 4097), device=DEV)
    P = lambda t: t.data_ptr()
    vote = lambda k, lds, top: lib.nsid_song_vote(P(I), k, P(big), lds, P(zero), P(one), 1, P(so), 8, 0, None, top, P(out_s), P(out_t),
                                                  P(out_n), None)
    assert vote(65, 65, 10) == -1 and vote(1, 4096, 33) == -1 and vote(1, 4097, 10) == -1 and vote(0, 1, 10) == -1
    assert vote(1, 0, 10) == -1 and vote(1, 1, 0) == -1
    vclf = lambda k, top: lib.nsid_song_vote_clf(P(I), k, P(big), P(off), P(one), P(zero), P(one), 1, P(so), 8, 0, None, 0.5, top,
                                                 P(out_s), P(out_t), P(out_n), None)
    assert vclf(65, 10) == -1 and vclf(1, 33) == -1 and vclf(0, 10) == -1
    assert lib.nsid_vote_candidates(P(I), -1, 0, 8, P(out_n), None) == -1
    assert sum(ops.launch_counters().values()) == 0


def test_baseline_model_identifies_without_rerank():
    """the ResNet-IBN baseline (d = 2048) through extract_fingerprints; it has no node matrices, so rerank=True is refused"""
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.fingerprint import extract_fingerprints
    from neuralsampleid_amd.identify import SampleIndex
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    from synth import synth_state
    model = BaselineModel({"arch": "resnet-ibn", "n_frames": 216}, ResNetIBN())
    sd = synth_state(model.state_dict())
    sd["encoder.global_pool.p"] = torch.full((1,), 2.5)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    specs = (torch.randn(6, 84, 216, generator=g).abs() * 2).to(DEV)
    idx = SampleIndex(model, device=DEV)
    assert idx.d == 2048
    for i in range(3):
        idx.add(f"b{i}", specs=specs[2 * i:2 * i + 2])
    assert torch.equal(idx.fingerprints[2:4], extract_fingerprints(model, specs[2:4]))
    assert idx.identify(specs=specs[2:3], k_probe=1, top=1).songs == ["b1"]
    with pytest.raises(NotImplementedError):
        SampleIndex(model, classifier=CrossAttentionClassifier(512, num_nodes=32).to(DEV).eval(), device=DEV).identify(
            specs=specs[:1], rerank=True)
