"""GPU: pair_sim against fp64, local_align against the oracle bit for bit, the two chained, planted occurrences through the kernels, and
SampleIndex.align / locate (fingerprints at d = 128 and d = 2048, and the classifier's scores)."""
import math

import numpy as np
import pytest
import torch

from locate_oracle import (PLANT_MIN_SCORE, PLANT_NOISE, PLANT_SEEDS, PLANT_SHAPE, PLANT_THETA, PLANTS, align_oracle, case, dyadic,
                           occurrences, plants_matched, smooth_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


@pytest.fixture(autouse=True)
def _fp32_switches():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _blocks(S, s_off, s_ld, q_len, x_len):
    """the pairs' matrices of a flat S, on the host"""
    S = S.cpu().numpy()
    out = []
    for o, ld, n, m in zip(*(np.asarray(a).tolist() for a in (s_off, s_ld, q_len, x_len))):
        out.append(S[o + np.arange(n)[:, None] * ld + np.arange(m)[None, :]] if n * m else np.zeros((n, m), np.float32))
    return out


def assert_align_equals_oracle(got, mats, theta, min_score, top, oracle_rows=None):
    """local_align's seven results against the oracle of every pair: scores as bit patterns, everything else exactly, unused slots too"""
    occ, sc, n_occ, row_h, row_j, row_org, row_off = got
    occ, sc, n_occ, row_h, row_j, row_org = (t.cpu().numpy() for t in (occ, sc, n_occ, row_h, row_j, row_org))
    assert occ.shape == (len(mats), top, 4) and sc.shape == (len(mats), top) and n_occ.shape == (len(mats),)
    assert row_h.size == sum(m.shape[0] for m in mats)
    over = 0
    for p, m in enumerate(mats):
        if m.shape[0] == 0 or m.shape[1] == 0:
            res = align_oracle(m, theta, min_score, top)
            want, rows = res[:3], res[3:]
        else:
            rows = align_oracle(m, theta)[3:] if oracle_rows is None else oracle_rows[p]
            want = occurrences(*rows, min_score, top)
        assert n_occ[p] == want[2], (p, m.shape)
        np.testing.assert_array_equal(occ[p], want[0], err_msg=f"pair {p} {m.shape}")
        np.testing.assert_array_equal(_bits(sc[p]), _bits(want[1]), err_msg=f"pair {p} {m.shape}")
        over += want[2] > top
        if m.shape[0] > 0:
            a, b = int(row_off[p]), int(row_off[p]) + m.shape[0]
            np.testing.assert_array_equal(_bits(row_h[a:b]), _bits(rows[0]), err_msg=f"pair {p} {m.shape}")
            np.testing.assert_array_equal(row_j[a:b], rows[1], err_msg=f"pair {p} {m.shape}")
            np.testing.assert_array_equal(row_org[a:b], rows[2], err_msg=f"pair {p} {m.shape}")
    return over


# ------------------------------------------------------------------------------------------------ pair_sim
SIM_SHAPES = [(1, 1, 16), (3, 2, 64), (33, 65, 128), (64, 31, 256), (19, 130, 2048), (5, 4096, 128), (4096, 5, 128)]


def _sim_call(d, shapes, seed):
    """pairs of the given (Lq, Lr) at width d in one call: non-zero starts, s_ld > x_len for every second pair, a sentinel everywhere"""
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(seed)
    q_len, x_len = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    q_start = 3 + np.cumsum(q_len + 2) - q_len
    x_start = 5 + np.cumsum(x_len + 1) - x_len
    q = rng.standard_normal((int(q_start[-1] + q_len[-1] + 4), d)).astype(np.float32)
    x = rng.standard_normal((int(x_start[-1] + x_len[-1] + 4), d)).astype(np.float32)
    s_ld = x_len + np.array([0 if p % 2 == 0 else 3 + p for p in range(len(shapes))])
    total = int((q_len * s_ld).sum())
    out = torch.full((total + 100,), SENTINEL, device=DEV)
    qd, xd = _dev(q), _dev(x)
    S, s_off, s_ld2 = ops.pair_sim(qd, xd, q_start, q_len, x_start, x_len, s_ld=s_ld, out=out)
    assert S is out and np.array_equal(s_ld2, s_ld) and np.array_equal(s_off, np.cumsum(q_len * s_ld) - q_len * s_ld)
    return q, x, qd, xd, q_start, q_len, x_start, x_len, s_off, s_ld, S


@pytest.mark.parametrize("d", [16, 64, 128, 256, 2048])
def test_pair_sim_against_fp64(d):
    from neuralsampleid_amd import ops
    shapes = [(lq, lr) for lq, lr, dd in SIM_SHAPES if dd == d] + [(7, 9), (32, 32), (1, 40)]
    before = ops.launch_counters()["pair_sim"]
    q, x, qd, xd, q_start, q_len, x_start, x_len, s_off, s_ld, S = _sim_call(d, shapes, d)
    assert ops.launch_counters()["pair_sim"] == before + 1                       # every pair in one launch
    host = S.cpu().numpy()
    written = np.zeros(host.size, dtype=bool)
    for p, (lq, lr) in enumerate(shapes):
        qq, xx = q[q_start[p]:q_start[p] + lq].astype(np.float64), x[x_start[p]:x_start[p] + lr].astype(np.float64)
        want = qq @ xx.T
        bound = 1.2e-6 * np.linalg.norm(qq, axis=1)[:, None] * np.linalg.norm(xx, axis=1)[None, :] + 1e-12
        idx = s_off[p] + np.arange(lq)[:, None] * s_ld[p] + np.arange(lr)[None, :]
        got = host[idx].astype(np.float64)
        assert (np.abs(got - want) <= bound).all(), (p, lq, lr, float((np.abs(got - want) / bound).max()))
        written[idx] = True
    # between x_len and s_ld, and past the last pair's last row: untouched
    assert (host[~written] == np.float32(SENTINEL)).all() and (~written).sum() >= 100
    assert not (host[written] == np.float32(SENTINEL)).any()
    # a pair alone gives the bits it gives inside the batch; two runs are bitwise equal
    for p in (0, len(shapes) - 1):
        alone, off1, ld1 = ops.pair_sim(qd, xd, [q_start[p]], [q_len[p]], [x_start[p]], [x_len[p]])
        assert off1.tolist() == [0] and ld1.tolist() == [x_len[p]]
        idx = s_off[p] + np.arange(q_len[p])[:, None] * s_ld[p] + np.arange(x_len[p])[None, :]
        np.testing.assert_array_equal(_bits(alone.cpu().numpy()), _bits(host[idx].reshape(-1)))
    again = _sim_call(d, shapes, d)[-1]
    assert torch.equal(again, S)


def test_pair_sim_element_does_not_depend_on_its_tile():
    """the same two rows at different places of different pairs: one chain, the same bits"""
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(7)
    for d in (128, 2048):
        q = rng.standard_normal((70, d)).astype(np.float32)
        x = rng.standard_normal((70, d)).astype(np.float32)
        q[0] = q[37] = q[69]
        x[0] = x[33] = x[68]
        S, s_off, s_ld = ops.pair_sim(_dev(q), _dev(x), [0, 30], [70, 40], [0, 20], [70, 50])
        a, b = _blocks(S, s_off, s_ld, [70, 40], [70, 50])
        ref = _bits(a[0, 0])
        for v in (a[37, 33], a[69, 68], a[0, 68], a[69, 0], b[7, 13], b[39, 48]):
            assert _bits(v) == ref


# ------------------------------------------------------------------------------------------------ local_align
ALIGN_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (31, 33), (33, 65), (64, 31), (65, 64), (300, 257), (5, 4096), (4096, 5)]


@pytest.fixture(scope="module")
def dyadic_pairs():
    """the shapes as pairs of one call plus an empty pair, with s_ld > x_len for some; the oracle's row results, computed once"""
    rng = np.random.default_rng(2024)
    mats = [dyadic(rng, lq, lr) for lq, lr in ALIGN_SHAPES]
    mats.insert(4, np.zeros((0, 9), np.float32))                     # an empty pair in the middle
    mats.append(np.zeros((6, 0), np.float32))
    q_len, x_len = np.array([m.shape[0] for m in mats]), np.array([m.shape[1] for m in mats])
    s_ld = x_len + np.array([(p % 3) * 5 for p in range(len(mats))])
    size = q_len * s_ld
    s_off = np.cumsum(size) - size + 11
    flat = np.full(int(size.sum()) + 11, np.nan, dtype=np.float32)    # what lies between the columns is never read: NaN would show
    for m, o, ld in zip(mats, s_off, s_ld):
        for i in range(m.shape[0]):
            flat[o + i * ld:o + i * ld + m.shape[1]] = m[i]
    rows = [align_oracle(m, 0.5)[3:] if m.size else None for m in mats]
    return mats, q_len, x_len, s_off, s_ld, flat, rows


@pytest.mark.parametrize("top", [1, 16, 64])
def test_local_align_equals_the_oracle_bit_for_bit(dyadic_pairs, top):
    from neuralsampleid_amd import ops
    mats, q_len, x_len, s_off, s_ld, flat, rows = dyadic_pairs
    S = _dev(flat)
    before = ops.launch_counters()["local_align"]
    got = ops.local_align(S, s_off, s_ld, q_len, x_len, 0.5, min_score=0.0, top=top)
    assert ops.launch_counters()["local_align"] == before + 1
    over = assert_align_equals_oracle(got, mats, 0.5, 0.0, top, rows)
    assert over >= 1                                                  # n_occ > top occurs (on the oracle's side)
    again = ops.local_align(S, s_off, s_ld, q_len, x_len, 0.5, min_score=0.0, top=top)
    for a, b in zip(got[:6], again[:6]):
        assert torch.equal(a, b)
    # a min_score that some occurrences meet exactly (dyadic sums): >= keeps them
    got = ops.local_align(S, s_off, s_ld, q_len, x_len, 0.5, min_score=0.75, top=top)
    assert_align_equals_oracle(got, mats, 0.5, 0.75, top, rows)
    kept_exact = sum(int((occurrences(*r, 0.75, 64)[1] == np.float32(0.75)).sum()) for r in rows if r is not None)
    assert kept_exact >= 1


def test_local_align_small_pairs_alone_take_the_narrow_workgroup(dyadic_pairs):
    """pairs of at most 1024 rows and columns run with 256 threads, larger ones with 1024: the results do not depend on it"""
    from neuralsampleid_amd import ops
    mats, q_len, x_len, s_off, s_ld, flat, rows = dyadic_pairs
    small = [p for p in range(len(mats)) if max(mats[p].shape) <= 1024]
    got = ops.local_align(_dev(flat), s_off[small], s_ld[small], q_len[small], x_len[small], 0.5, top=16)
    assert_align_equals_oracle(got, [mats[p] for p in small], 0.5, 0.0, 16, [rows[p] for p in small])


def test_pair_sim_then_local_align():
    """local_align on pair_sim's own output equals the oracle on that output"""
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(5)
    shapes = [(33, 65), (64, 31), (120, 300), (1, 1)]
    q_len, x_len = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    q_start, x_start = np.cumsum(q_len) - q_len, np.cumsum(x_len) - x_len
    q, x = smooth_rows(rng, int(q_len.sum()), 64), smooth_rows(rng, int(x_len.sum()), 64)
    for p in range(3):                                                # some rows in common, so that paths exist
        n = min(20, shapes[p][0], shapes[p][1])
        q[q_start[p] + 5:q_start[p] + 5 + n] = x[x_start[p] + 3:x_start[p] + 3 + n]
    S, s_off, s_ld = ops.pair_sim(_dev(q), _dev(x), q_start, q_len, x_start, x_len)
    got = ops.local_align(S, s_off, s_ld, q_len, x_len, 0.55, min_score=1.0, top=16)
    mats = _blocks(S, s_off, s_ld, q_len, x_len)
    assert_align_equals_oracle(got, mats, 0.55, 1.0, 16)
    n_occ = got[2].cpu().numpy()
    assert (n_occ[:3] >= 1).all()


def test_planted_occurrences_through_the_kernels():
    from neuralsampleid_amd import ops
    Lq, Lr, d = PLANT_SHAPE
    cases = [case(seed, Lq, Lr, d, PLANTS, PLANT_NOISE) for seed in PLANT_SEEDS]
    n = len(cases)
    q, x = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    S, s_off, s_ld = ops.pair_sim(_dev(q), _dev(x), np.arange(n) * Lq, [Lq] * n, np.arange(n) * Lr, [Lr] * n)
    got = ops.local_align(S, s_off, s_ld, [Lq] * n, [Lr] * n, PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16)
    mats = _blocks(S, s_off, s_ld, [Lq] * n, [Lr] * n)
    assert_align_equals_oracle(got, mats, PLANT_THETA, PLANT_MIN_SCORE, 16)
    occ, n_occ = got[0].cpu().numpy(), got[2].cpu().numpy()
    for p in range(n):
        assert plants_matched(occ[p], int(n_occ[p])), (p, occ[p, :max(int(n_occ[p]), 0)].tolist())


# ------------------------------------------------------------------------------------------------ SampleIndex
LOCATE_LQ = 300
LOCATE_PLANTS = [(15, 20, 12, 1.0), (100, 60, 16, 0.75), (190, 10, 10, 1.5), (270, 20, 12, 1.0)]
HOP_S, LEN_S = 0.5, 1.0


@pytest.fixture(scope="module", params=[128, 2048])
def planted_index(request):
    from neuralsampleid_amd.identify import SampleIndex
    d = request.param
    q, ref = case(1, LOCATE_LQ, 90, d, LOCATE_PLANTS, PLANT_NOISE)
    rng = np.random.default_rng(d)
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(smooth_rows(rng, 40, d)))
    songs = {"other 0": smooth_rows(rng, 70, d), "other 1": smooth_rows(rng, 33, d), "planted": ref, "other 2": smooth_rows(rng, 120, d),
             "other 3": smooth_rows(rng, 50, d), "other 4": smooth_rows(rng, 64, d), "other 5": smooth_rows(rng, 10, d)}
    for name, rows in songs.items():
        idx.add_rows(name, _dev(rows))
    return idx, _dev(q), songs


def _as_tuples(occs):
    return [(o.song, o.q_rows, o.r_rows, _bits(np.float32(o.score)).item()) for o in occs]


def test_align_returns_what_ops_return_for_each_song(planted_index):
    from neuralsampleid_amd import ops
    idx, q, songs = planted_index
    names = ["other 2", "planted", "other 5"]
    per_song, rows = idx.align(q, names, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, return_rows=True,
                               row_hop_s=HOP_S, row_len_s=LEN_S)
    assert len(per_song) == 3 and len(rows["chunks"]) == 1
    assert per_song[0] == [] and per_song[2] == []                    # a song without a plant: nothing above min_score
    x_start = [idx._song_rows[idx.code(n)][0] for n in names]
    x_len = [songs[n].shape[0] for n in names]
    S, s_off, s_ld = ops.pair_sim(q, idx.fingerprints, [0] * 3, [LOCATE_LQ] * 3, x_start, x_len)
    assert torch.equal(S, rows["chunks"][0][1])
    occ, sc, n_occ, *_ = (t.cpu().numpy() for t in ops.local_align(S, s_off, s_ld, [LOCATE_LQ] * 3, x_len, PLANT_THETA,
                                                                   PLANT_MIN_SCORE, 16)[:3])
    assert n_occ.tolist() == [0, 4, 0]
    assert plants_matched(occ[1], 4, LOCATE_PLANTS)
    assert _as_tuples(per_song[1]) == [("planted", (o[0], o[1]), (o[2], o[3]), _bits(s).item()) for o, s in zip(occ[1, :4].tolist(), sc[1, :4])]
    # the S rows of the planted song are the fingerprints' dot products
    mats = _blocks(S, s_off, s_ld, [LOCATE_LQ] * 3, x_len)
    q64, x64 = q.cpu().numpy().astype(np.float64), songs["planted"].astype(np.float64)
    # planted rows are nearly parallel, so the partial sums are as large as the norms allow: the worst-case bound of a sequential fp32
    # chain of d fused multiply-adds, d 2^-24 |q| |x| (a wrong row would be off by about 0.1)
    bound = q.shape[1] * 2.0 ** -24 * np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(x64, axis=1)[None, :] + 1e-12
    assert (np.abs(mats[1] - q64 @ x64.T) <= bound).all()
    # a small byte budget cuts the songs into chunks and changes nothing
    chunked, rows2 = idx.align(q, names, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, return_rows=True,
                               row_hop_s=HOP_S, row_len_s=LEN_S, s_budget_bytes=4 * LOCATE_LQ * 95)
    assert len(rows2["chunks"]) == 3 and chunked == per_song
    # times and stretch
    for o, (a, b, n, rate) in zip(sorted(per_song[1], key=lambda o: o.q_rows), LOCATE_PLANTS):
        (i0, i1), (j0, j1) = o.q_rows, o.r_rows
        assert o.q_time == (i0 * HOP_S, i1 * HOP_S + LEN_S) and o.r_time == (j0 * HOP_S, j1 * HOP_S + LEN_S)
        assert o.stretch == (j1 - j0) / (i1 - i0)
        di, dj = n - 1, int(round((n - 1) * rate))                    # each end within one row
        assert (dj - 2) / (di + 2) <= o.stretch <= (dj + 2) / (di - 2), (o, rate)
    by_rate = {rate: o.stretch for o, (_, _, _, rate) in zip(sorted(per_song[1], key=lambda o: o.q_rows), LOCATE_PLANTS)}
    assert by_rate[0.75] < by_rate[1.0] < by_rate[1.5]
    # without a row timing the times are None
    assert all(o.q_time is None and o.r_time is None for o in idx.align(q, ["planted"], threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE)[0])


def test_locate_finds_the_planted_song_through_windows(planted_index):
    from neuralsampleid_amd import ops
    idx, q, songs = planted_index
    assert LOCATE_LQ * 20 > ops.VOTE_MAX_CAND                         # more than one window at k_probe = 20
    with pytest.raises(ValueError):
        idx.identify(fp=q, k_probe=20)                                # the whole query as one vote is refused
    cand = idx._candidates(q, None, 20, 5, None, False)
    assert "planted" in cand and len(cand) == 5 and len(set(cand)) == 5
    occs = idx.locate(fp=q, k_probe=20, n_songs=5, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, row_hop_s=HOP_S, row_len_s=LEN_S)
    want = idx.align(q, ["planted"], threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, row_hop_s=HOP_S, row_len_s=LEN_S)[0]
    assert occs == want and len(occs) == 4                            # the other candidates hold nothing above min_score
    assert [o.score for o in occs] == sorted((o.score for o in occs), reverse=True)
    # named songs skip the search
    before = ops.launch_counters()
    assert idx.locate(fp=q, songs=["planted", "other 0"], threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, row_hop_s=HOP_S,
                      row_len_s=LEN_S) == want
    after = ops.launch_counters()
    assert after["flat_l2_topk"] == before["flat_l2_topk"] and after["pair_sim"] == before["pair_sim"] + 1
    # exclude removes a song from the candidates
    assert "planted" not in idx._candidates(q, None, 20, 5, "planted", False)
    assert idx.locate(fp=q, k_probe=20, n_songs=5, exclude="planted", threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE) == []


@pytest.mark.parametrize("N", [1, 32])
def test_align_on_classifier_scores(N):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.identify import CLF_THRESHOLD, SampleIndex
    torch.manual_seed(100 + N)
    clf = CrossAttentionClassifier(512, num_nodes=N).to(DEV).eval()
    g = torch.Generator().manual_seed(N)
    rng = np.random.default_rng(N)
    nodes = {n: torch.randn(s, 512, N, generator=g).to(DEV) for n, s in (("a", 20), ("b", 9), ("q", 12))}
    idx = SampleIndex(None, classifier=clf, device=DEV)
    idx.add_rows("a", _dev(smooth_rows(rng, 20, 128)), nodes["a"])
    idx.add_rows("b", _dev(smooth_rows(rng, 15, 128)), nodes["b"])     # fewer node matrices than rows
    idx.add_rows("c", _dev(smooth_rows(rng, 8, 128)))                  # none at all
    q = _dev(smooth_rows(rng, 12, 128))
    with torch.no_grad():
        want_S = {n: clf.pair_scores(nodes["q"], nodes[n]) for n in ("a", "b")}
    theta = float(torch.cat([want_S["a"].reshape(-1), want_S["b"].reshape(-1)]).median())
    per_song, rows = idx.align(q, ["a", "b", "c"], threshold=theta, nodes=nodes["q"], rerank=True, return_rows=True, top=64)
    codes, S, s_off, s_ld, x_len = rows["chunks"][0][:5]
    assert x_len.tolist() == [20, 9, 0]                               # columns exist only for rows with node matrices
    mats = _blocks(S, s_off, s_ld, [12, 12, 12], x_len)
    for m, n in zip(mats, ("a", "b")):
        assert torch.equal(torch.from_numpy(m).to(DEV), want_S[n])    # the agreement test_rerank_gpu.py asserts: the same bits
    total = 0
    for p, m in enumerate(mats):
        occ, sc, n_occ, *_ = align_oracle(m, theta, 0.0, 64)
        assert [(o.q_rows, o.r_rows, _bits(np.float32(o.score)).item()) for o in per_song[p]] == \
            [((o[0], o[1]), (o[2], o[3]), _bits(s).item()) for o, s in zip(occ[:n_occ].tolist(), sc[:n_occ])]
        total += n_occ
    assert total >= 1 and per_song[2] == []
    # the default threshold of a re-rank is the classifier's
    dflt = idx.align(q, ["a"], nodes=nodes["q"], rerank=True, top=64)[0]
    occ, sc, n_occ, *_ = align_oracle(mats[0], CLF_THRESHOLD, 0.0, 64)
    assert [(o.q_rows, o.r_rows) for o in dflt] == [((o[0], o[1]), (o[2], o[3])) for o in occ[:n_occ].tolist()]


def test_refusals_launch_nothing():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.default_rng(3)
    idx = SampleIndex(None, device=DEV)
    idx.add_rows("planted", _dev(smooth_rows(rng, 60, 128)))
    q = _dev(smooth_rows(rng, LOCATE_LQ, 128))
    x = idx.fingerprints
    S = torch.zeros(72, device=DEV)
    before = ops.launch_counters()

    def refused(exc, fn, *a, **k):
        with pytest.raises(exc):
            fn(*a, **k)
        assert ops.launch_counters() == before

    refused(ValueError, ops.pair_sim, q, x, [0], [4097], [0], [5])                     # past the limits
    refused(ValueError, ops.pair_sim, q, x, [0], [5], [0], [4097])
    refused(ValueError, ops.pair_sim, q, x, [290], [11], [0], [5])                     # leaves q
    refused(ValueError, ops.pair_sim, q, x, [0], [5], [x.shape[0] - 4], [5])           # leaves x
    refused(ValueError, ops.pair_sim, q, x, [0], [5], [0], [5], s_ld=[4])              # s_ld < x_len
    refused(ValueError, ops.pair_sim, q, x[:, :64], [0], [5], [0], [5])                # d differs
    refused(ValueError, ops.pair_sim, q, x, [0], [5], [0], [5], out=torch.zeros(24, device=DEV))
    refused(RuntimeError, ops.pair_sim, q.cpu(), x, [0], [5], [0], [5])
    refused(ValueError, ops.local_align, S, [0], [9], [8], [9], 0.5, top=0)
    refused(ValueError, ops.local_align, S, [0], [9], [8], [9], 0.5, top=65)
    refused(ValueError, ops.local_align, S, [0], [9], [8], [9], float("nan"))
    refused(ValueError, ops.local_align, S, [0], [9], [8], [9], 0.5, min_score=float("nan"))
    refused(ValueError, ops.local_align, S, [1], [9], [8], [9], 0.5)                   # the block leaves S
    refused(ValueError, ops.local_align, S, [0], [8], [8], [9], 0.5)                   # s_ld < x_len
    refused(ValueError, ops.local_align, S, [0], [1], [4097], [1], 0.5)
    refused(ValueError, ops.local_align, S, [0], [4097], [1], [4097], 0.5)
    refused(ValueError, ops.local_align, S, [0], [9], [-1], [9], 0.5)
    refused(RuntimeError, ops.local_align, S.cpu(), [0], [9], [8], [9], 0.5)
    refused(RuntimeError, ops.local_align, S.double(), [0], [9], [8], [9], 0.5)
    refused(ValueError, idx.align, q, ["planted"])                                      # no threshold without rerank
    refused(ValueError, idx.locate, fp=q)
    refused(RuntimeError, idx.align, q, ["planted"], rerank=True)                       # no classifier
    refused(KeyError, idx.align, q, ["no such song"], threshold=0.5)
    refused(KeyError, idx.locate, fp=q, threshold=0.5, exclude="no such song")
    refused(ValueError, idx.align, q, ["planted"], threshold=0.5, top=65)
    refused(ValueError, idx.align, q[:, :64].contiguous(), ["planted"], threshold=0.5)
    refused(ValueError, idx.locate, fp=q, threshold=0.5, k_probe=0)
    refused(RuntimeError, idx.align, q.cpu(), ["planted"], threshold=0.5)
    # an empty song list and an empty call launch nothing and return nothing
    assert idx.align(q, [], threshold=0.5) == []
    occ, sc, n_occ, *_ = ops.local_align(S, [], [], [], [], 0.5)
    assert occ.shape == (0, 16, 4) and n_occ.numel() == 0
    assert ops.launch_counters() == before
