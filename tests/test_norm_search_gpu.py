"""GPU: the normalised candidate search (nsid_flat_norm_topk, csrc/search.hip; FlatL2Index.search_norm; SampleIndex norm_search=True)
against tests/norm_search_oracle.py: Z as bits and I exactly on every path the plain search has, the cell of ops.pair_sim(norm=) bit
for bit, ties, NaN, padding, ranges, batch independence, and the retrieval hub case end to end on every seed."""
import numpy as np
import pytest
import torch

import norm_search_oracle as ns
from diag_vote_oracle import diag_vote
from score_norm_oracle import chain_dot, norm_cells

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device=DEV, dtype=dtype)          # a copy: the oracle's cached arrays are read-only


def _rows(rng, n, d):
    return (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)


def _stats(rng, n):
    """any statistics will do for the kernel: means around the dots' scale, inverse deviations of a few units"""
    return (0.1 * rng.standard_normal(n)).astype(np.float32), rng.uniform(0.5, 3.0, n).astype(np.float32)


def _took():
    from neuralsampleid_amd import _lib
    return _lib.lib.nsid_debug_last_kernel().decode()


def _search(q, x, qs, xs, k, lo=None, hi=None):
    """ops.flat_norm_topk on host arrays -> (Z, I) numpy"""
    from neuralsampleid_amd import ops
    ex = None if lo is None else (_dev(np.asarray(lo), torch.int32), _dev(np.asarray(hi), torch.int32))
    Z, I = ops.flat_norm_topk(_dev(q), _dev(x), tuple(_dev(v) for v in qs + xs), k, ex)
    torch.cuda.synchronize()
    return Z.cpu().numpy(), I.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


def _splits(nq, nx):
    """the number of database splits of the narrow phase 1 (csrc/search.hip nsid_l2_plan): 2048 waves over the query tiles, splits of
    at least 1024 rows, each a multiple of 32"""
    nqt = (nq + 31) // 32
    S = min((2048 + nqt - 1) // nqt, max(1, nx // 1024))
    c = ((nx + S - 1) // S + 31) // 32 * 32
    return max(1, (nx + c - 1) // c)


TWO_SPLITS = next(nx for nx in range(1, 1 << 14) if _splits(33, nx) > 1)


def test_the_smallest_database_of_two_splits():
    assert TWO_SPLITS == 2048 and _splits(1, TWO_SPLITS) == _splits(33, TWO_SPLITS) == 2 and _splits(33, TWO_SPLITS - 1) == 1


# ---------------------------------------------------------------------------------------------------- bitwise against the oracle
@pytest.mark.parametrize("d", [16, 128, 256])
def test_split_kernel_equals_the_oracle(d):
    """a cell's bits depend on its two rows alone, so one oracle matrix of 33 x 2048 serves every (nq, nx, k) as a corner of it"""
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(100 + d)
    q, x = _rows(rng, 33, d), _rows(rng, TWO_SPLITS, d)
    x[7], x[1500] = x[3], x[3]                                         # equal scores further down
    qs, xs = _stats(rng, 33), _stats(rng, TWO_SPLITS)
    for v in xs:
        v[7] = v[1500] = v[3]
    z = norm_cells(chain_dot(q, x), *qs, *xs)
    before = ops.launch_counters()
    calls = 0
    for nq in (1, 33):
        for nx in (1, 31, 33, 1000, TWO_SPLITS):
            for k in (1, 20, 64, min(nx + 3, 64) if nx < 64 else None):
                if k is None:
                    continue
                got = _search(q[:nq], x[:nx], tuple(v[:nq] for v in qs), tuple(v[:nx] for v in xs), k)
                calls += 1
                assert _took() == "l2_topk_split_kernel<norm>"
                want = ns.norm_topk(z[:nq, :nx], k)
                assert _same(got, want), (d, nq, nx, k, np.argwhere(got[1] != want[1])[:4].tolist())
                assert (got[1][:, min(k, nx):] == -1).all() and np.isneginf(got[0][:, min(k, nx):]).all()
    got = _search(q, x[:20], qs, tuple(v[:20] for v in xs), 64)       # k > nx at a k the loop did not take
    assert _same(got, ns.norm_topk(z[:, :20], 64)) and (got[1][:, 20:] == -1).all()
    after = ops.launch_counters()
    assert after["flat_norm_topk"] - before["flat_norm_topk"] == calls + 1
    for c in ("flat_norm_topk_wide", "flat_l2_topk", "flat_l2_topk_excl", "flat_l2_topk_wide", "row_sqnorm"):
        assert after[c] == before[c], c


@pytest.mark.parametrize("nq,form", [(8, "l2_topk_wide_kernel<1,norm>"), (130, "l2_topk_wide_kernel<4,norm>")])
def test_wide_kernel_equals_the_oracle(nq, form):
    from neuralsampleid_amd import ops
    d, nx = 320, 300
    rng = np.random.default_rng(nq)
    q, x = _rows(rng, nq, d), _rows(rng, nx, d)
    qs, xs = _stats(rng, nq), _stats(rng, nx)
    z = norm_cells(chain_dot(q, x), *qs, *xs)
    before = ops.launch_counters()
    for k in (1, 20, 64):
        got = _search(q, x, qs, xs, k)
        assert _took() == form
        want = ns.norm_topk(z, k)
        assert _same(got, want), (nq, k, np.argwhere(got[1] != want[1])[:4].tolist())
    after = ops.launch_counters()
    assert after["flat_norm_topk"] - before["flat_norm_topk"] == after["flat_norm_topk_wide"] - before["flat_norm_topk_wide"] == 3
    assert after["flat_l2_topk_wide"] == before["flat_l2_topk_wide"]


# ---------------------------------------------------------------------------------------------------- against the library itself
@pytest.mark.parametrize("d,nq,nx", [(128, 40, 2500), (320, 40, 700)])
def test_scores_are_the_cells_of_pair_sim_norm(d, nq, nx):
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(d)
    q, x = _dev(_rows(rng, nq, d)), _dev(_rows(rng, nx, d))
    cohort = _dev(_rows(rng, 64, d))
    norm = ops.cohort_stats(q, cohort) + ops.cohort_stats(x, cohort)
    Z, I = ops.flat_norm_topk(q, x, norm, 20)
    S, s_off, s_ld = ops.pair_sim(q, x, [0], [nq], [0], [nx], norm=norm)
    cells = S[: nq * nx].reshape(nq, nx)
    assert torch.equal(Z.view(torch.int32), torch.gather(cells, 1, I).view(torch.int32))
    order = torch.sort(cells, dim=1, descending=True, stable=True)           # the library's own cells, sorted: the same lists
    assert torch.equal(I, order.indices[:, :20]) and (Z[:, :-1] >= Z[:, 1:]).all()


# ---------------------------------------------------------------------------------------------------- ties, NaN, padding
@pytest.mark.parametrize("d,nx", [(128, 2500), (320, 700)])
def test_ties_nan_and_padding(d, nx):
    rng = np.random.default_rng(7 + d)
    x = _rows(rng, nx, d)
    dup = [5, 100, nx // 2 + 9, nx - 1]                                # in both splits / several column blocks
    for j in dup[1:]:
        x[j] = x[5]
    q = np.stack([x[5] + 1e-3 * _rows(rng, 1, d)[0]] * 3)
    qs = (np.zeros(3, np.float32), np.ones(3, np.float32))
    xs = (np.zeros(nx, np.float32), np.ones(nx, np.float32))           # z = s: the duplicates' equal scores are the largest
    Z, I = _search(q, x, qs, xs, 6)
    assert I[0][:4].tolist() == dup and Z[0][0] == Z[0][3] and (I == I[0]).all()
    xs[0][100] = np.nan                                                # that row's z is NaN: it does not compete
    Z, I = _search(q, x, qs, xs, 6)
    assert I[0][:3].tolist() == [5, dup[2], nx - 1] and not (I == 100).any()
    assert _same((Z, I), ns.norm_topk(norm_cells(chain_dot(q, x), *qs, *xs), 6))
    Z, I = _search(q, x, qs, (np.full(nx, np.nan, np.float32), xs[1]), 6)
    assert (I == -1).all() and np.isneginf(Z).all()
    Z, I = _search(q, x, (np.array([0, np.nan, 0], np.float32), qs[1]), (np.zeros(nx, np.float32), xs[1]), 6)
    assert (I[1] == -1).all() and np.isneginf(Z[1]).all() and I[0][:4].tolist() == dup and I[2][:4].tolist() == dup


# ---------------------------------------------------------------------------------------------------- ranges
@pytest.mark.parametrize("d,nq,nx,edge,form", [(128, 33, 2100, 1056, "l2_topk_split_kernel<excl,norm>"),
                                               (320, 20, 700, 256, "l2_topk_wide_kernel<1,excl,norm>"),
                                               (320, 130, 700, 128, "l2_topk_wide_kernel<4,excl,norm>")])
def test_ranges_equal_the_oracle_without_the_rows(d, nq, nx, edge, form):
    """edge: where phase 1 cuts the database (the narrow kernel's two splits of 1056 rows; the wide forms' column blocks)"""
    rng = np.random.default_rng(nq + d)
    q, x = _rows(rng, nq, d), _rows(rng, nx, d)
    qs, xs = _stats(rng, nq), _stats(rng, nx)
    z = norm_cells(chain_dot(q, x), *qs, *xs)
    kinds = [(0, 0), (nx, nx), (0, nx), (0, 31), (31, 33), (edge - 16, edge + 14), (edge, min(2 * edge, nx)), (edge, nx), (nx - 1, nx),
             (5, nx - 3), (40, 7), (-5, 2 ** 31 - 1)]                  # a whole split; lo >= hi; 8 rows remain; everything
    lo = [kinds[(i + d) % len(kinds)][0] for i in range(nq)]
    hi = [kinds[(i + d) % len(kinds)][1] for i in range(nq)]
    for k in (1, 20, 64):
        got = _search(q, x, qs, xs, k, lo, hi)
        assert _took() == form
        want = ns.norm_topk(z, k, lo, hi)
        assert _same(got, want), (d, nq, k, np.argwhere(got[1] != want[1])[:4].tolist())
    none = _search(q, x, qs, xs, 20, [0] * nq, [0] * nq)
    assert _same(none, _search(q, x, qs, xs, 20)) and _same(none, ns.norm_topk(z, 20))


# ---------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("d,nx", [(128, 2500), (320, 700)])
def test_a_row_does_not_depend_on_the_batch(d, nx):
    rng = np.random.default_rng(d + 1)
    q, x = _rows(rng, 33, d), _rows(rng, nx, d)
    qs, xs = _stats(rng, 33), _stats(rng, nx)
    Z, I = _search(q, x, qs, xs, 20)
    for i in (0, 17, 32):
        alone = _search(q[i:i + 1], x, tuple(v[i:i + 1] for v in qs), xs, 20)
        assert _same(alone, (Z[i:i + 1], I[i:i + 1])), i


# ---------------------------------------------------------------------------------------------------- the hub case end to end
def _hub_index(h, songs=None):
    from neuralsampleid_amd.identify import SampleIndex
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(h["dummy"]))
    for c, rows in enumerate(h["songs"] if songs is None else songs):
        idx.add_rows(f"song{c}", _dev(rows))
    idx.set_cohort(size=ns.HUB_COHORT)
    return idx


def _plant_ok(o):
    return o.song == "song2" and all(abs(got - want) <= 1 for got, want in zip(o.q_rows + o.r_rows, (0, 31, 10, 41)))


@pytest.mark.parametrize("seed", list(ns.HUB_SEEDS))
def test_hub_case_end_to_end(seed):
    h = ns.hub(seed)
    idx = _hub_index(h)
    q = _dev(h["query"])
    L, k = q.shape[0], ns.HUB_K
    # the vote equals the oracle's vote over the oracle's lists
    dv = idx.diag_votes(q, [0], [L], k_probe=k, top=5, norm_search=True)
    _, I = ns.norm_topk(h["z"], k)
    want = diag_vote(I, [0], [L], h["song_of"], h["n_dummy"], None, 16, 5)
    got = (dv.codes, dv.counts, dv.i_lo, dv.i_hi, dv.r_lo, dv.r_hi, dv.n_songs)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w), (g, w)
    kw = dict(fp=q, threshold=ns.HUB_THETA, min_score=ns.HUB_MIN_SCORE, vote="diagonal", normalize=True, n_songs=3, k_probe=k)
    found = idx.locate(norm_search=True, **kw)
    assert found and _plant_ok(found[0]), found[:2]
    assert not any(o.song == "song2" for o in idx.locate(norm_search=False, **kw))
    assert not any(o.song == "song2" for o in idx.locate(**kw))


def test_scanner_in_pieces_equals_scan():
    h = ns.hub(0)
    idx = _hub_index(h)
    q = _dev(h["query"])
    kw = dict(threshold=ns.HUB_THETA, min_score=ns.HUB_MIN_SCORE, vote="diagonal", normalize=True, norm_search=True, n_songs=3,
              k_probe=ns.HUB_K, window_rows=16)
    whole = idx.scan(fp=q, **kw)
    sc = idx.scanner(**kw)
    for a, b in ((0, 5), (5, 25), (25, 48)):
        sc.push(q[a:b])
    assert sc.finish() == whole and sc.stats["windows"] == 3
    assert whole and whole[0].song == "song2"
    plain = idx.scanner(**{**kw, "norm_search": False})                # the keyword off: the windows' search is the L2 search
    plain.push(q)
    plain.finish()
    assert [t["vote_codes"] for t in plain.trace] != [t["vote_codes"] for t in sc.trace]


def _occ_key(o):
    return (o.song, o.score, o.q_rows, o.r_rows)


def test_links_equal_the_locate_loop():
    """a three-song catalogue in which song1 samples song0 under a generic component, and song2 is a hub song"""
    h = ns.hub(1)
    rng = np.random.default_rng(11)
    s0, s1, s2 = h["songs"][0].copy(), h["songs"][1].copy(), h["songs"][5].copy()
    u = h["songs"][5][20].astype(np.float64)                           # a generic row stands in for the direction u
    for t in range(24):
        v = s0[5 + t].astype(np.float64) + 0.5 * rng.standard_normal(ns.HUB_D) / np.sqrt(ns.HUB_D) + 1.5 * u
        s1[20 + t] = (v / np.linalg.norm(v)).astype(np.float32)
    idx = _hub_index(h, [s0, s1, s2])
    kw = dict(threshold=ns.HUB_THETA, min_score=ns.HUB_MIN_SCORE, vote="diagonal", normalize=True, norm_search=True, k_probe=ns.HUB_K)
    links = idx.links(**kw)
    assert links.skipped == []
    for c, name in enumerate(idx.names):
        lo, n, _ = idx._song_rows[c]
        want = idx.locate(fp=idx.fingerprints[lo:lo + n], leave_out=name, **kw)
        assert [_occ_key(o) for o in links.occurrences[name]] == [_occ_key(o) for o in want], name
        assert not any(o.song == name for o in want)
    assert any(o.song == "song0" for o in links.occurrences["song1"]) and any(o.song == "song1" for o in links.occurrences["song0"])
    blocks = idx.links(block_rows=64, names=["song2", "song0", "song1"], **kw)        # one song per block, out of add order
    for name in idx.names:
        assert [_occ_key(o) for o in blocks.occurrences[name]] == [_occ_key(o) for o in links.occurrences[name]], name


def test_index_statistics_are_cached_and_dropped():
    from neuralsampleid_amd import ops
    h = ns.hub(2)
    idx = _hub_index(h, h["songs"][:3])
    q = _dev(h["query"])
    idx.diag_votes(q, [0], [48], norm_search=True)
    n0 = idx.n_dummy + idx.n_ref
    assert idx._istat_done == n0 and idx._stat_done == idx.n_ref
    keep = tuple(t[:n0].clone() for t in idx._istat)
    direct = ops.cohort_stats(idx._index.xb, idx._cohort)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, direct))
    for a, b in zip(keep, idx._stat):                                  # the ref part is the resident statistics, the same bits
        assert torch.equal(a[idx.n_dummy:].view(torch.int32), b[: idx.n_ref].view(torch.int32))
    before = ops.launch_counters()["cohort_stats"]
    idx.diag_votes(q, [0], [48], norm_search=True)
    assert ops.launch_counters()["cohort_stats"] == before + 1         # the query rows alone: nothing of the index is computed again
    idx.add_rows("late", _dev(h["songs"][7]))
    idx.diag_votes(q, [0], [48], norm_search=True)
    n1 = idx.n_dummy + idx.n_ref
    assert n1 == n0 + 64 and idx._istat_done == n1
    assert ops.launch_counters()["cohort_stats"] == before + 3         # the query rows and the 64 new rows
    for a, b in zip(keep, idx._istat):
        assert torch.equal(a.view(torch.int32), b[:n0].view(torch.int32))
    late = ops.cohort_stats(_dev(h["songs"][7]), idx._cohort)
    for a, b in zip(late, idx._istat):
        assert torch.equal(a.view(torch.int32), b[n0:n1].view(torch.int32))
    idx.set_cohort(size=256)
    assert idx._istat is None and idx._istat_done == 0 and idx._stat is None
    idx.diag_votes(q, [0], [48], norm_search=True)
    assert idx._istat_done == n1 and not torch.equal(idx._istat[0][:n0], keep[0])


def test_search_norm_of_the_index_and_its_refusal():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    rng = np.random.default_rng(5)
    q, x = _rows(rng, 9, 128), _rows(rng, 400, 128)
    qs, xs = _stats(rng, 9), _stats(rng, 400)
    norm = tuple(_dev(v) for v in qs + xs)
    index = FlatL2Index(128, DEV)
    index.add(_dev(x))
    z = norm_cells(chain_dot(q, x), *qs, *xs)
    Z, I = index.search_norm(_dev(q), 20, norm)
    assert _same((Z.cpu().numpy(), I.cpu().numpy()), ns.norm_topk(z, 20))
    lo, hi = [0, 10, 399, 0, 5, 0, 0, 200, 7], [0, 50, 400, 400, 5, 1, 0, 300, 9]
    Z, I = index.search_norm(_dev(q), 20, norm, exclude=(lo, hi))
    assert _same((Z.cpu().numpy(), I.cpu().numpy()), ns.norm_topk(z, 20, lo, hi))
    D0, I0 = index.search(_dev(q), 20)                                 # the exact search is what it was
    assert torch.equal(I0, ops.flat_l2_topk(_dev(q), _dev(x), ops.row_sqnorm(_dev(x)), 20)[1])
    pre = FlatL2Index(128, DEV, prefilter=True)
    pre.add(_dev(x))
    with pytest.raises(ValueError, match="pre-filter"):
        pre.search_norm(_dev(q), 20, norm)
