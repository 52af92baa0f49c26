"""GPU: the leave-one-out search (nsid_flat_l2_topk_excl, csrc/search.hip) against the plain entry, bit for bit. The expected value never
comes from the code under test: it is ops.flat_l2_topk (pinned to the reference's golden by tests/test_search_gpu.py) over the database
with the row's range deleted, torch.cat([x[:lo], x[hi:]]) with the matching norms, the ids mapped back (tests/search_excl_oracle.py)."""
import numpy as np
import pytest
import torch

from search_excl_oracle import groups, map_back

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_MAX = 2 ** 31 - 1


def _rows(g, n, d, scale=1.0):
    return (torch.randn(n, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)).float()


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _expected(q, x, xn, k, lo, hi):
    """one plain search per distinct range over the compacted database, ids mapped back: (D, I) on the device"""
    from neuralsampleid_amd import ops
    nx = x.shape[0]
    D = torch.empty((q.shape[0], k), device=DEV, dtype=torch.float32)
    I = torch.empty((q.shape[0], k), device=DEV, dtype=torch.int64)
    for (a, b), rows in groups(lo, hi, nx):
        r = torch.from_numpy(rows).to(DEV)
        xc = torch.cat([x[:a], x[b:]]).contiguous()
        xnc = torch.cat([xn[:a], xn[b:]]).contiguous()
        Dc, Ic = ops.flat_l2_topk(q[r].contiguous(), xc, xnc, k)
        D[r] = Dc
        I[r] = torch.from_numpy(map_back(Ic.cpu().numpy(), a, b)).to(DEV)
    return D, I


def _same(got, want):
    return torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def _ranges(nx, edge, k):
    """the ranges of the issue for a database of nx rows whose phase-1 work is cut at multiples of `edge`"""
    return [(0, 0), (nx, nx), (0, nx), (0, 31), (31, 33), (32, 64), (edge - 16, edge + 14), (edge, min(2 * edge, nx)), (nx - 1, nx),
            (5, nx - 3),                                   # 8 rows remain: a padded tail at k = 20 and 64
            (200, 260), (200, 260)]                        # the rows' planted nearest neighbours lie inside (see _case)


def _case(nq, nx, d, k, edge, seed):
    """queries near database rows; row i takes range (i + seed) % 12, so one 32-row tile mixes them all; the rows of the last two kinds
    get q_i + 1e-3 noise planted inside their range, which the plain search puts first"""
    g = torch.Generator().manual_seed(seed)
    x = _rows(g, nx, d)
    q = x[torch.randint(0, nx, (nq,), generator=g)] + _rows(g, nq, d, 0.3)
    rs = _ranges(nx, edge, k)
    kind = [(i + seed) % len(rs) for i in range(nq)]
    planted = []
    for i in range(nq):
        if kind[i] >= 10 and 200 + i < 260:
            x[200 + i] = q[i] + _rows(g, 1, d, 1e-3)[0]
            planted.append((i, 200 + i))
    lo, hi = [rs[t][0] for t in kind], [rs[t][1] for t in kind]
    return q.to(DEV), x.to(DEV), lo, hi, planted


def _run_case(nq, nx, d, k, edge, seed, counter):
    from neuralsampleid_amd import ops
    q, x, lo, hi, planted = _case(nq, nx, d, k, edge, seed)
    xn = ops.row_sqnorm(x)
    before = ops.launch_counters()
    got = ops.flat_l2_topk_excl(q, x, xn, k, _i32(lo), _i32(hi))
    after = ops.launch_counters()
    assert after["flat_l2_topk_excl"] == before["flat_l2_topk_excl"] + 1 and after["flat_l2_topk"] == before["flat_l2_topk"]
    assert after["flat_l2_topk_wide_excl"] - before["flat_l2_topk_wide_excl"] == (1 if counter == "wide" else 0)
    want = _expected(q, x, xn, k, lo, hi)
    assert _same(got, want), (nq, nx, d, k, (got[1] != want[1]).nonzero()[:4].tolist())
    I = got[1].cpu().numpy()
    for i in range(nq):
        real = I[i][I[i] >= 0]
        assert not ((real >= lo[i]) & (real < hi[i])).any(), i
        assert real.size == min(k, nx - max(0, min(hi[i], nx) - max(lo[i], 0))), i
    if planted:                                            # the plain search does put the planted rows first
        _, Ip = ops.flat_l2_topk(q, x, xn, 1)
        assert [int(Ip[i, 0]) for i, _ in planted] == [j for _, j in planted]
    return len(planted)


@pytest.mark.parametrize("nx", [2100, 4200])               # 2 and 4 splits of 1056 rows (the plan is not exported: both are run)
@pytest.mark.parametrize("d", [16, 128, 256])
def test_narrow_forms_equal_the_plain_search_without_the_rows(d, nx):
    planted = 0
    for nq in (1, 33, 65):
        for k in (1, 20, 64):
            planted += _run_case(nq, nx, d, k, 1056, nq + k + d, "narrow")
    assert planted >= 6


@pytest.mark.parametrize("nq", [20, 130])                  # the 32 x 256 form (WQ = 1), and the 128 x 128 form over two query blocks
@pytest.mark.parametrize("d", [320, 2048])
def test_wide_forms_equal_the_plain_search_without_the_rows(d, nq):
    planted = 0
    for k in (1, 20, 64):
        planted += _run_case(nq, 700, d, k, 256 if nq == 20 else 128, nq + k + d, "wide")
    assert planted >= 3


@pytest.mark.parametrize("d", [128, 2048])
def test_exact_ties_go_to_the_smaller_surviving_id(d):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(2)
    nx = 5000 if d == 128 else 1500
    x = _rows(g, nx, d)
    dup = [5, 100, 1200, nx - 1]
    for j in dup[1:]:
        x[j] = x[5]
    q = torch.stack([x[5] + 1e-3 * _rows(g, 1, d)[0]] * 4)
    x, q = x.to(DEV), q.to(DEV)
    xn = ops.row_sqnorm(x)
    lo, hi = [0, 90, 0, 6], [0, 1201, 101, nx]             # nothing; the two in the middle; the first two; all but the first
    D, I = ops.flat_l2_topk_excl(q, x, xn, 4, _i32(lo), _i32(hi))
    assert I[0].tolist() == dup and I[1, :2].tolist() == [5, nx - 1] and I[2, :2].tolist() == [1200, nx - 1]
    assert I[3].tolist()[:1] == [5] and not (I[3, 1:] == 100).any()
    assert D[0, 0] == D[0, 3] == D[1, 1] == D[2, 0] == D[2, 1] == D[3, 0]
    assert _same((D, I), _expected(q, x, xn, 4, lo, hi))


@pytest.mark.parametrize("nq,nx,d", [(65, 2100, 128), (130, 700, 2048), (20, 700, 320)])
def test_empty_ranges_equal_the_plain_entry(nq, nx, d):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(11)
    x = _rows(g, nx, d).to(DEV)
    q = _rows(g, nq, d).to(DEV)
    xn = ops.row_sqnorm(x)
    plain = ops.flat_l2_topk(q, x, xn, 20)
    z = torch.zeros(nq, dtype=torch.int32, device=DEV)
    assert _same(ops.flat_l2_topk_excl(q, x, xn, 20, z, z), plain)
    assert _same(ops.flat_l2_topk_excl(q, x, xn, 20, z + nx, z + nx), plain)
    assert _same(ops.flat_l2_topk_excl(q, x, xn, 20, z + 40, z + 7), plain)


def test_index_search_with_empty_ranges_equals_search():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(12)
    idx = FlatL2Index(128, DEV)
    idx.add(_rows(g, 3000, 128).numpy())
    q = _rows(g, 70, 128)
    before = ops.launch_counters()
    D, I = idx.search(q.numpy(), 20)
    mid = ops.launch_counters()
    De, Ie = idx.search(q.numpy(), 20, exclude=(np.zeros(70, np.int64), np.zeros(70, np.int64)))
    after = ops.launch_counters()
    assert np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32))
    assert (mid["flat_l2_topk"], mid["flat_l2_topk_excl"]) == (before["flat_l2_topk"] + 1, before["flat_l2_topk_excl"])
    assert (after["flat_l2_topk"], after["flat_l2_topk_excl"]) == (mid["flat_l2_topk"], mid["flat_l2_topk_excl"] + 1)
    # song-like ranges through the index, tensors in and out
    lo = (torch.arange(70) * 40) % 2900
    Dt, It = idx.search(q.to(DEV), 20, exclude=(lo, lo + 100))
    want = _expected(q.to(DEV), idx.xb, ops.row_sqnorm(idx.xb), 20, lo.tolist(), (lo + 100).tolist())
    assert _same((Dt, It), want)


def test_batch_invariance_and_run_to_run():
    """row r searched alone with its range is bitwise row r of a 4099-row call (a different split of the database); two calls agree"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(6)
    nx, nq = 50003, 4099
    x = _rows(g, nx, 128).to(DEV)
    xn = ops.row_sqnorm(x)
    pick = torch.randint(0, nx, (nq,), generator=g)
    q = (x[pick].cpu() + _rows(g, nq, 128, 0.5)).to(DEV)
    lo = (pick - 150).clamp(0, nx).to(torch.int32).to(DEV)          # every row's own neighbourhood: its nearest row is left out
    hi = (pick + 150).clamp(0, nx).to(torch.int32).to(DEV)
    D, I = ops.flat_l2_topk_excl(q, x, xn, 20, lo, hi)
    D2, I2 = ops.flat_l2_topk_excl(q, x, xn, 20, lo, hi)
    assert torch.equal(I, I2) and torch.equal(D.view(torch.int32), D2.view(torch.int32))
    assert not ((I >= lo[:, None]) & (I < hi[:, None])).any() and (I >= 0).all()
    for r in (0, 31, 32, 1000, 4098):
        Dr, Ir = ops.flat_l2_topk_excl(q[r:r + 1], x, xn, 20, lo[r:r + 1], hi[r:r + 1])
        assert torch.equal(Ir[0], I[r]) and torch.equal(Dr[0].view(torch.int32), D[r].view(torch.int32)), r
    D19, I19 = ops.flat_l2_topk_excl(q[1000:1019], x, xn, 20, lo[1000:1019], hi[1000:1019])
    assert torch.equal(I19, I[1000:1019]) and torch.equal(D19.view(torch.int32), D[1000:1019].view(torch.int32))
    rows = [0, 31, 32, 1000, 4098]
    want = _expected(q[rows].contiguous(), x, xn, 20, lo[rows].tolist(), hi[rows].tolist())
    assert _same((D[rows], I[rows]), want)


@pytest.mark.parametrize("nq,nx,d", [(40, 2100, 128), (40, 700, 2048)])
def test_garbage_ranges_are_only_compared(nq, nx, d):
    """any pair of ints: -5 .. INT_MAX leaves nothing, lo > hi leaves everything, a range that sticks out is cut at the database"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(13)
    x = _rows(g, nx, d).to(DEV)
    q = _rows(g, nq, d).to(DEV)
    xn = ops.row_sqnorm(x)
    kinds = [(-5, INT_MAX), (INT_MAX, -5), (-INT_MAX - 1, INT_MAX), (INT_MAX, INT_MAX), (-5, 50), (nx - 50, INT_MAX), (-INT_MAX - 1, -1),
             (7, 7)]
    lo, hi = [kinds[i % 8][0] for i in range(nq)], [kinds[i % 8][1] for i in range(nq)]
    D, I = ops.flat_l2_topk_excl(q, x, xn, 20, _i32(lo), _i32(hi))
    torch.cuda.synchronize()
    plain = ops.flat_l2_topk(q, x, xn, 20)
    for i in range(nq):
        t = i % 8
        if t in (0, 2):
            assert (I[i] == -1).all() and torch.isinf(D[i]).all() and (D[i] > 0).all()
        elif t in (1, 3, 6, 7):
            assert torch.equal(I[i], plain[1][i]) and torch.equal(D[i].view(torch.int32), plain[0][i].view(torch.int32))
    assert _same((D, I), _expected(q, x, xn, 20, lo, hi))


def test_bad_arguments_return_einval_and_launch_nothing():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import DEFINES, lib
    einval = DEFINES["NSID_EINVAL"]
    x = torch.zeros(64, 128, device=DEV)
    xn = torch.zeros(64, device=DEV)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    D = torch.empty(64, 65, device=DEV)
    I = torch.empty(64, 65, device=DEV, dtype=torch.int64)
    ops.launch_counters(reset=True)

    def c_call(d=128, k=5, lo=z.data_ptr(), hi=z.data_ptr(), q=x.data_ptr(), Dp=D.data_ptr(), wsb=ws.numel()):
        return lib.nsid_flat_l2_topk_excl(q, d, 64, x.data_ptr(), d, 64, xn.data_ptr(), xn.data_ptr(), lo, hi, d, k, Dp, I.data_ptr(),
                                          ws.data_ptr(), wsb, None)
    for kw in ({"k": 0}, {"k": 65}, {"d": 120}, {"d": 8}, {"d": 272}, {"d": 2112}, {"lo": None}, {"hi": None}, {"q": None}, {"Dp": None},
               {"wsb": 16}):
        assert c_call(**kw) == einval, kw
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.flat_l2_topk_excl(x, x, xn, k, z, z)
    for bad in (z[:63], z.long(), z.cpu(), z.float(), z.view(8, 8), None, [0] * 64):
        with pytest.raises(ValueError):
            ops.flat_l2_topk_excl(x, x, xn, 5, bad, z)
        with pytest.raises(ValueError):
            ops.flat_l2_topk_excl(x, x, xn, 5, z, bad)
    y = torch.zeros(64, 24, device=DEV)
    with pytest.raises(ValueError):
        ops.flat_l2_topk_excl(y, y, xn, 5, z, z)
    c = ops.launch_counters()
    assert c["flat_l2_topk_excl"] == c["flat_l2_topk_wide_excl"] == c["flat_l2_topk"] == c["row_sqnorm"] == 0
    assert c_call() == 0 and ops.launch_counters()["flat_l2_topk_excl"] == 1
    torch.cuda.synchronize()
