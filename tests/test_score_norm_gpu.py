"""GPU: cohort score normalisation. cohort_stats and pair_sim_norm against the oracle bit for bit (the sums formed from the GPU's own
pair_sim scores, which is what the rule says s_m is), plain pair_sim untouched, and normalize=True through SampleIndex: align on the
hub case, scanner, links, long songs, paths and the refusals."""
import numpy as np
import pytest
import torch

import score_norm_oracle as sn
from locate_oracle import align_oracle, smooth_rows
from test_links_gpu import as_tuples, build_index, make_catalogue, rows_of
from test_links_gpu import _name as song_name
from test_locate_gpu import SIM_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
KW_NORM = dict(threshold=sn.NORM_THETA, min_score=sn.NORM_MIN_SCORE, top=16)


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


def _scores(x, c):
    """the GPU's own pair_sim matrix of all rows of x against all rows of c, on the host"""
    from neuralsampleid_amd import ops
    n, M = x.shape[0], c.shape[0]
    starts = np.arange(0, n, ops.ALIGN_MAX_ROWS)                  # one pair per ALIGN_MAX_ROWS rows: the blocks follow each other
    S, _, _ = ops.pair_sim(x, c, starts, np.minimum(n - starts, ops.ALIGN_MAX_ROWS), np.zeros_like(starts), np.full_like(starts, M),
                           long_songs=M > ops.ALIGN_MAX_COLS)
    return S.cpu().numpy().reshape(n, M)


def _oracle_stats(x, c):
    return sn.cohort_stats(_scores(x, c))


# ------------------------------------------------------------------------------------------------ cohort_stats
# every n of {1, 31, 33, 70}, M of {32, 33, 255, 257, 1000} and d of {16, 128, 256, 320, 2048} at least once, and 17 chunks
STAT_SHAPES = [(1, 32, 16), (31, 33, 128), (33, 255, 256), (70, 257, 320), (33, 1000, 2048), (70, 4101, 128)]


@pytest.mark.parametrize("n,M,d", STAT_SHAPES)
def test_cohort_stats_bit_for_bit(n, M, d):
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(1000 * n + M + d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    c = (rng.standard_normal((M, d)) + 0.3 * rng.standard_normal(d)).astype(np.float32)          # a common direction: mu is not ~0
    xd, cd = _dev(x), _dev(c)
    before = ops.launch_counters()["cohort_stats"]
    mu, rs = ops.cohort_stats(xd, cd)
    assert ops.launch_counters()["cohort_stats"] == before + 1
    assert mu.shape == rs.shape == (n,) and mu.dtype == rs.dtype == torch.float32 and mu.is_cuda
    S = _scores(xd, cd)
    want_mu, want_rs = sn.cohort_stats(S)
    np.testing.assert_array_equal(_bits(mu.cpu().numpy()), _bits(want_mu))
    np.testing.assert_array_equal(_bits(rs.cpu().numpy()), _bits(want_rs))
    # against fp64 directly: the bound test_pair_sim_against_fp64 uses per element, averaged over the cohort
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    mu64 = (x64 @ c64.T).mean(axis=1)
    bound = 1.2e-6 * np.linalg.norm(x64, axis=1) * np.linalg.norm(c64, axis=1).mean() + 1e-12
    err = np.abs(mu.cpu().numpy().astype(np.float64) - mu64)
    print(f"(n, M, d) = {(n, M, d)}: largest |mu - mu64| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    sd64 = (x64 @ c64.T).std(axis=1)
    assert np.abs(rs.cpu().numpy() * sd64 - 1).max() < 1e-4
    # a row alone, at another position of another batch, and on a second run: the same bits
    i = n // 2
    other = rng.standard_normal((45, d)).astype(np.float32)
    other[37] = x[i]
    alone = ops.cohort_stats(xd[i:i + 1], cd)
    moved = ops.cohort_stats(_dev(other), cd)
    again = ops.cohort_stats(xd, cd)
    for got in (alone[0][0], moved[0][37], again[0][i]):
        assert _bits(got.cpu().numpy()) == _bits(want_mu[i])
    for got in (alone[1][0], moved[1][37], again[1][i]):
        assert _bits(got.cpu().numpy()) == _bits(want_rs[i])
    assert torch.equal(again[0], mu) and torch.equal(again[1], rs)


def test_cohort_stats_takes_strided_rows_and_refuses_the_rest():
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(5)
    wide = _dev(rng.standard_normal((40, 192)).astype(np.float32))
    c = _dev(rng.standard_normal((64, 128)).astype(np.float32))
    x = wide[:, :128]                                            # row stride 192
    mu, rs = ops.cohort_stats(x, c)
    ref = ops.cohort_stats(x.contiguous(), c)
    assert torch.equal(mu, ref[0]) and torch.equal(rs, ref[1])
    empty = ops.cohort_stats(x[:0], c)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    before = ops.launch_counters()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cohort_stats(x.cpu(), c)
    with pytest.raises(RuntimeError):
        ops.cohort_stats(x.double(), c)
    with pytest.raises(ValueError, match="outside"):
        ops.cohort_stats(x, c[:31])
    with pytest.raises(ValueError, match="limits"):
        ops.cohort_stats(wide[:, :120], _dev(np.zeros((64, 120), np.float32)))
    with pytest.raises(ValueError, match="!="):
        ops.cohort_stats(x, _dev(np.zeros((64, 64), np.float32)))
    assert ops.launch_counters() == before


# ------------------------------------------------------------------------------------------------ pair_sim_norm
NORM_SHAPES = [s + (False,) for s in SIM_SHAPES if 4096 not in s[:2]] + [(40, 4100, 128, True)]


def _pairs_call(lq, lr, d, long_songs):
    """two pairs, (lq, lr) and (7, 9), at non-zero starts, s_ld > x_len on the second, a sentinel everywhere: once through pair_sim
    and once through pair_sim_norm with arbitrary statistics"""
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(lq + lr + d)
    q_len, x_len = np.array([lq, 7]), np.array([lr, 9])
    q_start = 3 + np.cumsum(q_len + 2) - q_len
    x_start = 5 + np.cumsum(x_len + 1) - x_len
    q = rng.standard_normal((int(q_start[-1] + q_len[-1] + 4), d)).astype(np.float32)
    x = rng.standard_normal((int(x_start[-1] + x_len[-1] + 4), d)).astype(np.float32)
    s_ld = x_len + np.array([0, 4])
    total = int((q_len * s_ld).sum())
    qd, xd = _dev(q), _dev(x)
    stats = [rng.standard_normal(q.shape[0]), rng.uniform(0.5, 40.0, q.shape[0]), rng.standard_normal(x.shape[0]),
             rng.uniform(0.5, 40.0, x.shape[0])]
    stats = [v.astype(np.float32) for v in stats]
    out = {}
    for key in ("raw", "norm"):
        buf = torch.full((total + 100,), SENTINEL, device=DEV)
        norm = tuple(_dev(v) for v in stats) if key == "norm" else None
        S, s_off, _ = ops.pair_sim(qd, xd, q_start, q_len, x_start, x_len, s_ld=s_ld, out=buf, long_songs=long_songs, norm=norm)
        assert S is buf
        out[key] = S.cpu().numpy()
    return out, stats, q_start, q_len, x_start, x_len, s_off, s_ld


@pytest.mark.parametrize("lq,lr,d,long_songs", NORM_SHAPES)
def test_pair_sim_norm_bit_for_bit(lq, lr, d, long_songs):
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    out, stats, q_start, q_len, x_start, x_len, s_off, s_ld = _pairs_call(lq, lr, d, long_songs)
    after = ops.launch_counters()
    assert after["pair_sim_norm"] == before["pair_sim_norm"] + 1 and after["pair_sim"] == before["pair_sim"] + 1
    written = np.zeros(out["raw"].size, dtype=bool)
    for p in range(2):
        idx = s_off[p] + np.arange(q_len[p])[:, None] * s_ld[p] + np.arange(x_len[p])[None, :]
        a, b = slice(q_start[p], q_start[p] + q_len[p]), slice(x_start[p], x_start[p] + x_len[p])
        want = sn.norm_cells(out["raw"][idx], stats[0][a], stats[1][a], stats[2][b], stats[3][b])
        np.testing.assert_array_equal(_bits(out["norm"][idx]), _bits(want), err_msg=f"pair {p}")
        written[idx] = True
    for host in out.values():                                    # between x_len and s_ld, and past the last pair: untouched
        assert (host[~written] == np.float32(SENTINEL)).all() and (~written).sum() >= 100
        assert not (host[written] == np.float32(SENTINEL)).any()


def test_plain_pair_sim_is_the_unchanged_entry():
    """norm=None goes through nsid_pair_sim itself: the bits of a direct call of the entry on the same tables, its counter counts and
    pair_sim_norm's does not; and they are the oracle's chain"""
    from neuralsampleid_amd import _lib, ops
    rng = np.random.default_rng(11)
    for d in (128, 320):
        q, x = rng.standard_normal((70, d)).astype(np.float32), rng.standard_normal((45, d)).astype(np.float32)
        qd, xd = _dev(q), _dev(x)
        q_start, q_len, x_start, x_len = np.array([2, 0]), np.array([60, 33]), np.array([1, 5]), np.array([40, 35])
        before = ops.launch_counters()
        S, s_off, s_ld = ops.pair_sim(qd, xd, q_start, q_len, x_start, x_len, norm=None)
        mid = ops.launch_counters()
        assert mid["pair_sim"] == before["pair_sim"] + 1 and mid["pair_sim_norm"] == before["pair_sim_norm"]
        tiles = ops.pair_sim_tiles(q_len, x_len)
        t32 = _dev(np.stack([q_start, q_len, x_len, s_ld]).astype(np.int32))
        t64 = _dev(np.stack([x_start, s_off]).astype(np.int64))
        tl = _dev(tiles)
        direct = torch.full_like(S, SENTINEL)
        p = lambda t: t.data_ptr()
        _lib.call("nsid_pair_sim", p(qd), d, 70, p(xd), d, 45, d, p(t32[0]), p(t32[1]), p(t64[0]), p(t32[2]), p(t64[1]), p(t32[3]), 2,
                  p(tl), tiles.shape[0], p(direct), direct.numel(), torch.cuda.current_stream().cuda_stream)
        after = ops.launch_counters()
        assert after["pair_sim"] == mid["pair_sim"] + 1 and after["pair_sim_norm"] == mid["pair_sim_norm"]
        assert torch.equal(S.view(torch.int32), direct.view(torch.int32))
        host = S.cpu().numpy()
        want = sn.chain_dot(q[2:62], x[1:41])
        np.testing.assert_array_equal(_bits(host[:60 * 40].reshape(60, 40)), _bits(want))


def test_pair_sim_norm_refusals():
    from neuralsampleid_amd import ops
    q, x = _dev(np.ones((20, 128), np.float32)), _dev(np.ones((30, 128), np.float32))
    ok = (torch.zeros(20, device=DEV), torch.ones(20, device=DEV), torch.zeros(30, device=DEV), torch.ones(30, device=DEV))
    ops.pair_sim(q, x, [0], [20], [0], [30], norm=ok)
    before = ops.launch_counters()
    for k in range(4):                                           # an array shorter than the rows it indexes
        bad = list(ok)
        bad[k] = bad[k][:-1]
        with pytest.raises(ValueError, match="one entry per row"):
            ops.pair_sim(q, x, [0], [5], [0], [5], norm=tuple(bad))
    with pytest.raises(ValueError, match="norm must be"):
        ops.pair_sim(q, x, [0], [5], [0], [5], norm=ok[:3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pair_sim(q, x, [0], [5], [0], [5], norm=(ok[0].cpu(),) + ok[1:])
    with pytest.raises(RuntimeError, match="float32"):
        ops.pair_sim(q, x, [0], [5], [0], [5], norm=(ok[0].double(),) + ok[1:])
    assert ops.launch_counters() == before


# ------------------------------------------------------------------------------------------------ SampleIndex on the hub case
def _hub_index(seed):
    from neuralsampleid_amd.identify import SampleIndex
    q, song, cohort = sn.hub_case(seed)
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(cohort))
    idx.add_rows("song", _dev(song))
    idx.set_cohort()
    return idx, _dev(q), _dev(song), _dev(cohort)


def _occ_array(occs, top=16):
    occ = np.full((top, 4), -1, dtype=np.int32)
    sc = np.zeros(top, dtype=np.float32)
    for n, o in enumerate(occs):
        occ[n] = o.q_rows + o.r_rows
        sc[n] = o.score
    return occ, sc


@pytest.fixture(scope="module")
def hub0():
    return _hub_index(0)


def test_align_normalized_equals_the_oracle_on_the_hub_case(hub0):
    from neuralsampleid_amd import ops
    idx, q, song, cohort = hub0
    assert idx._cohort.shape == (sn.HUB_COHORT, 128) and torch.equal(idx._cohort, cohort)          # positions floor(m n / M) = m
    before = ops.launch_counters()
    per_song, rows = idx.align(q, ["song"], return_rows=True, normalize=True, **KW_NORM)
    after = ops.launch_counters()
    assert after["pair_sim_norm"] == before["pair_sim_norm"] + 1 and after["pair_sim"] == before["pair_sim"]
    S_norm = sn.norm_cells(_scores(q, song), *_oracle_stats(q, cohort), *_oracle_stats(song, cohort))
    chunk = rows["chunks"][0]
    np.testing.assert_array_equal(_bits(chunk[1].cpu().numpy().reshape(100, 90)), _bits(S_norm))
    want = align_oracle(S_norm, sn.NORM_THETA, sn.NORM_MIN_SCORE, 16)
    occ, sc = _occ_array(per_song[0])
    np.testing.assert_array_equal(occ, want[0])
    np.testing.assert_array_equal(_bits(sc), _bits(want[1]))
    assert want[2] == len(per_song[0]) >= 3 and sn.plants_found(want[0], want[2]) and not sn.in_box(want[0], want[2])
    # without normalize: the call of before this option, on nsid_pair_sim
    mid = ops.launch_counters()
    raw = idx.align(q, ["song"], threshold=sn.RAW_THETA, min_score=sn.RAW_MIN_SCORE, top=16)
    end = ops.launch_counters()
    assert end["pair_sim"] == mid["pair_sim"] + 1 and end["pair_sim_norm"] == mid["pair_sim_norm"]
    want_raw = align_oracle(_scores(q, song), sn.RAW_THETA, sn.RAW_MIN_SCORE, 16)
    occ, sc = _occ_array(raw[0])
    np.testing.assert_array_equal(occ, want_raw[0])
    np.testing.assert_array_equal(_bits(sc), _bits(want_raw[1]))


@pytest.mark.parametrize("seed", list(sn.HUB_SEEDS))
def test_hub_condition_on_the_device(seed, hub0):
    idx, q, _, _ = hub0 if seed == 0 else _hub_index(seed)
    raw = idx.align(q, ["song"], threshold=sn.RAW_THETA, min_score=sn.RAW_MIN_SCORE, top=16)[0]
    nrm = idx.align(q, ["song"], normalize=True, **KW_NORM)[0]
    raw_occ, nrm_occ = _occ_array(raw)[0], _occ_array(nrm)[0]
    print(f"seed {seed}: raw {len(raw)} occurrences, {len(sn.in_box(raw_occ, len(raw)))} in the box; normalised {len(nrm)}, "
          f"{len(sn.in_box(nrm_occ, len(nrm)))} in the box")
    assert sn.plants_found(raw_occ, len(raw)) and len(sn.in_box(raw_occ, len(raw))) >= 1
    assert sn.plants_found(nrm_occ, len(nrm)) and len(sn.in_box(nrm_occ, len(nrm))) == 0


# ------------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("cut", [7, 150])
def test_scanner_normalized_equals_align(hub0, cut):
    idx, q, _, _ = hub0
    want = idx.align(q, ["song"], normalize=True, **KW_NORM)[0]
    sc = idx.scanner(songs=["song"], window_rows=24, normalize=True, **KW_NORM)
    for a in range(0, q.shape[0], cut):
        sc.push(q[a:a + cut])
    got = sc.finish()
    assert sc.stats["windows"] == 5 and len(got) >= 3
    assert as_tuples(got) == as_tuples(want)
    raw = idx.scanner(songs=["song"], window_rows=24, threshold=sn.NORM_THETA, min_score=sn.NORM_MIN_SCORE)      # raw cells never reach 7
    raw.push(q)
    assert raw.finish() == []


@pytest.fixture(scope="module")
def catalogue():
    dummy, songs = make_catalogue()
    idx = build_index(dummy, songs)
    rng = np.random.Generator(np.random.PCG64(99))
    idx.set_cohort(rows=_dev(smooth_rows(rng, 300, 128)))
    return idx, songs


def test_links_normalized_equal_locate_and_the_cached_statistics(catalogue):
    from neuralsampleid_amd import ops
    idx, songs = catalogue
    kw = dict(k_probe=20, n_songs=11, normalize=True, **KW_NORM)
    names = [song_name(c) for c in (0, 3, 2, 6)]
    before = ops.launch_counters()
    links = idx.links(names=names, **kw)
    after = ops.launch_counters()
    assert after["pair_sim_norm"] > before["pair_sim_norm"] and after["pair_sim"] == before["pair_sim"]
    assert after["cohort_stats"] == before["cohort_stats"] + 1               # the resident rows, once; links has no other rows
    found = 0
    for name in names:
        want = idx.locate(fp=rows_of(idx, name), leave_out=name, **kw)
        assert as_tuples(links.occurrences[name]) == as_tuples(want)
        found += len(want)
    assert found >= 4 and any(o.song == song_name(3) for o in links.occurrences[song_name(0)])
    # the cached resident statistics are what cohort_stats gives for those rows; later adds compute the new rows only
    mu, rs = idx._stat[0][: idx.n_ref], idx._stat[1][: idx.n_ref]
    assert idx._stat_done == idx.n_ref
    got = idx.cohort_stats(idx.fingerprints[100:417])
    assert torch.equal(got[0], mu[100:417]) and torch.equal(got[1], rs[100:417])
    want_mu, want_rs = _oracle_stats(idx.fingerprints[100:417].contiguous(), idx._cohort)
    np.testing.assert_array_equal(_bits(got[0].cpu().numpy()), _bits(want_mu))
    np.testing.assert_array_equal(_bits(got[1].cpu().numpy()), _bits(want_rs))
    n_before, keep = idx.n_ref, (mu.clone(), rs.clone())
    idx.add_rows("late", idx.fingerprints[40:75].clone())
    count = ops.launch_counters()["cohort_stats"]
    idx.align(idx.fingerprints[:50].contiguous(), ["late"], normalize=True, **KW_NORM)
    assert ops.launch_counters()["cohort_stats"] == count + 2               # the 35 new resident rows and the query's rows
    assert idx._stat_done == idx.n_ref == n_before + 35
    assert torch.equal(idx._stat[0][:n_before], keep[0]) and torch.equal(idx._stat[1][:n_before], keep[1])
    assert torch.equal(idx._stat[0][n_before: idx.n_ref], keep[0][40:75])
    # a new cohort drops them
    idx.set_cohort(rows=idx._cohort[:64])
    assert idx._stat is None and idx._stat_done == 0


def test_long_song_normalized_equals_the_oracle():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.Generator(np.random.PCG64(5))
    song, cohort, q = smooth_rows(rng, 4100, 128), smooth_rows(rng, 64, 128), smooth_rows(rng, 40, 128)
    for t in range(16):
        v = song[4070 + t] + 0.5 * rng.standard_normal(128) / np.sqrt(128)
        q[10 + t] = (v / np.linalg.norm(v)).astype(np.float32)
    idx = SampleIndex(None, device=DEV, long_songs=True)
    idx.add_dummy(_dev(cohort))
    idx.add_rows("long", _dev(song))
    qd = _dev(q)
    before = ops.launch_counters()
    got = idx.align(qd, ["long"], normalize=True, **KW_NORM)[0]
    after = ops.launch_counters()
    assert after["local_align_panels"] == before["local_align_panels"] + 1 and after["pair_sim_norm"] == before["pair_sim_norm"] + 1
    assert idx._cohort.shape == (64, 128)                          # the default cohort, taken by the call
    S_norm = sn.norm_cells(_scores(qd, _dev(song)), *_oracle_stats(qd, _dev(cohort)), *_oracle_stats(_dev(song), _dev(cohort)))
    want = align_oracle(S_norm, sn.NORM_THETA, sn.NORM_MIN_SCORE, 16)
    occ, sc = _occ_array(got)
    np.testing.assert_array_equal(occ, want[0])
    np.testing.assert_array_equal(_bits(sc), _bits(want[1]))
    assert want[2] == len(got) >= 1 and any(abs(o[0] - 10) <= 1 and abs(o[2] - 4070) <= 1 for o in want[0].tolist())


# ------------------------------------------------------------------------------------------------ paths
def test_paths_normalized(hub0):
    idx, q, song, cohort = hub0
    occs = idx.align(q, ["song"], normalize=True, **KW_NORM)[0]
    assert len(occs) >= 3
    paths = idx.paths(q, occs, sn.NORM_THETA, normalize=True)            # its own score check passes
    S_norm = sn.norm_cells(_scores(q, song), *_oracle_stats(q, cohort), *_oracle_stats(song, cohort))
    for p, o in zip(paths, occs):
        pi, pj, h = sn.box_path(S_norm, sn.NORM_THETA, o.q_rows[0], o.q_rows[1], o.r_rows[0], o.r_rows[1])
        assert pi is not None and _bits(h) == _bits(np.float32(o.score))
        np.testing.assert_array_equal(p.q_rows, pi)
        np.testing.assert_array_equal(p.r_rows, pj)
        np.testing.assert_array_equal(_bits(p.scores), _bits(S_norm[pi, pj]))
    with pytest.raises(ValueError, match="is not an occurrence of these rows"):
        idx.paths(q, occs, sn.NORM_THETA, normalize=False)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(hub0):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    idx, q, song, cohort = hub0
    bare = SampleIndex(None, device=DEV)
    bare.add_dummy(cohort[:31])
    bare.add_rows("song", song)
    before = ops.launch_counters()
    with pytest.raises(ValueError, match="rerank"):
        idx.align(q, ["song"], normalize=True, rerank=True, **KW_NORM)
    with pytest.raises(ValueError, match="rerank"):
        idx.locate(fp=q, normalize=True, rerank=True, **KW_NORM)
    with pytest.raises(ValueError, match="no default"):
        idx.align(q, ["song"], normalize=True)                     # threshold keeps having none
    keep = idx._cohort
    with pytest.raises(ValueError, match="d = 128"):
        idx.set_cohort(rows=_dev(np.zeros((64, 64), np.float32)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        idx.set_cohort(rows=torch.zeros(64, 128))
    with pytest.raises(ValueError, match="outside"):
        idx.set_cohort(rows=cohort[:31])
    with pytest.raises(ValueError, match="outside"):
        idx.set_cohort(size=31)
    assert idx._cohort is keep
    for call in (lambda: bare.align(q, ["song"], normalize=True, **KW_NORM),
                 lambda: bare.locate(fp=q, normalize=True, **KW_NORM),
                 lambda: bare.scanner(songs=["song"], normalize=True, **KW_NORM),
                 lambda: bare.links(normalize=True, **KW_NORM),
                 lambda: bare.cohort_stats(q),
                 lambda: bare.set_cohort()):
        with pytest.raises(RuntimeError, match="set_cohort"):
            call()
    assert ops.launch_counters() == before
    bare.set_cohort(rows=cohort[:32])                              # then it runs
    assert isinstance(bare.align(q, ["song"], normalize=True, **KW_NORM)[0], list)
