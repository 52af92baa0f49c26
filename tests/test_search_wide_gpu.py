"""GPU: exact flat-L2 search at 256 < d <= 2048 (the LDS-staged wide kernel of csrc/search.hip) against fp64 brute force, with the
tie / padding / batch / run-to-run invariants of tests/test_search_gpu.py at d = 2048, and the row norms and sequence scores at wide d."""
import numpy as np
import pytest
import torch

from test_search_gpu import _fp64_dist, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eps(q, x):
    """fp32 error bound of D, the form of test_search_gpu._eps: the f32-MFMA dot is within 3.5e-7 sum|q x| of fp64 at K = 4096
    (the measured figure for the longest chain published, d <= 2048 here), taken x8 as there: 2.8e-6 in place of 1.2e-6"""
    qn = q.double().norm(dim=1)
    xm = float(x.double().norm(dim=1).max()) if x.shape[0] else 0.0
    return (2.8e-6 * (qn * qn + xm * xm + 2 * qn * xm) + 1e-12).to(DEV)


def _check_topk(q, x, k, D, I):
    nq, nx = q.shape[0], x.shape[0]
    kk = min(k, nx)
    assert D.shape == (nq, k) and I.shape == (nq, k) and I.dtype == torch.int64 and D.dtype == torch.float32
    if k > nx:
        assert (I[:, nx:] == -1).all() and torch.isinf(D[:, nx:]).all() and (D[:, nx:] > 0).all()
    if kk == 0:
        return
    Ik, Dk = I[:, :kk], D[:, :kk].double()
    assert (Ik >= 0).all() and (Ik < nx).all()
    assert (Dk[:, 1:] >= Dk[:, :-1]).all(), "D not ascending"
    ref = _fp64_dist(q, x)
    eps = _eps(q, x)[:, None]
    got = ref.gather(1, Ik)
    err = float((Dk - got).abs().max())
    print(f"max |D - fp64| = {err:.3g}, bound >= {float(eps.min()):.3g}")
    assert ((Dk - got).abs() <= eps).all(), err
    kth = ref.topk(kk, dim=1, largest=False).values[:, -1:]
    # every returned id lies within eps of the fp64 k-th; every id clearly inside the fp64 top-k is returned; no id twice
    assert (got <= kth + 2 * eps).all()
    hit = torch.zeros_like(ref, dtype=torch.bool)
    hit.scatter_(1, Ik, True)
    assert not ((ref < kth - 2 * eps) & ~hit).any()
    assert int(hit.sum()) == nq * kk, "duplicate ids"


CASES = [  # (nq, nx, d, k): the smallest wide d (no multiple of 128) and the largest; query tiles of 1, 19, 33 rows and two 128-row
    # blocks (130); a partial last database tile (20, 1000, 4099), several splits (4099, 65537); k at both ends
    (1, 1, 320, 1),
    (19, 20, 2048, 5),
    (33, 1000, 512, 20),
    (130, 4099, 2048, 64),
    (19, 65537, 2048, 20),
    (1, 4099, 1024, 64),
]


@pytest.mark.parametrize("nq,nx,d,k", CASES)
def test_flat_l2_topk_wide_vs_fp64(nq, nx, d, k):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(nq * 7 + nx + d + k)
    x = _rows(g, nx, d).to(DEV)
    q = (x[torch.randint(0, nx, (nq,), generator=g)].cpu() + _rows(g, nq, d, 0.3)).to(DEV)
    ops.launch_counters(reset=True)
    D, I = ops.flat_l2_topk(q, x, ops.row_sqnorm(x), k)
    torch.cuda.synchronize()
    assert ops.launch_counters()["flat_l2_topk_wide"] == 1
    _check_topk(q, x, k, D, I)


@pytest.mark.parametrize("nx,k", [(20, 64), (1, 5), (0, 3)])
def test_k_above_nx_pads(nx, k):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(5)
    x = _rows(g, nx, 2048).to(DEV)
    q = _rows(g, 5, 2048).to(DEV)
    D, I = ops.flat_l2_topk(q, x, ops.row_sqnorm(x), k)
    _check_topk(q, x, k, D, I)
    assert (I[:, nx:] == -1).all() and torch.isinf(D[:, nx:]).all() and (D[:, nx:] > 0).all()


def test_exact_ties_and_self_match():
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(2)
    x = _rows(g, 5000, 2048)
    x[100] = x[5]
    x[3000] = x[5]
    x[4999] = x[5]
    idx = FlatL2Index(2048, DEV)
    idx.add(x.numpy())
    q = torch.stack([x[5] + 1e-3 * _rows(g, 1, 2048)[0], x[17], x[4000]]).numpy()
    D, I = idx.search(q, 8)
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    assert list(I[0, :4]) == [5, 100, 3000, 4999]
    assert D[0, 0] == D[0, 1] == D[0, 2] == D[0, 3]
    assert I[1, 0] == 17 and I[2, 0] == 4000 and D[1, 0] < 1e-5 and D[2, 0] < 1e-5


def test_zero_rows_and_zero_query():
    """rows zeroed by the NaN -> 0 load: a zero query ranks the zero database rows first, smaller id first, at distance 0"""
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(3)
    x = _rows(g, 3000, 2048)
    zero = [7, 1234, 2999]
    x[zero] = 0.0
    idx = FlatL2Index(2048, DEV)
    idx.add(x.to(DEV))
    D, I = idx.search(torch.zeros(2, 2048, device=DEV), 5)
    assert I[:, :3].cpu().tolist() == [zero, zero] and (D[:, :3] == 0).all()
    assert (D[:, 3:] > 0).all()


def test_several_adds_equal_one():
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(4)
    x = _rows(g, 9001, 2048).numpy()
    q = _rows(g, 40, 2048).numpy()
    one = FlatL2Index(2048, DEV)
    one.add(x)
    many = FlatL2Index(2048, DEV)
    for a, b in ((0, 1), (1, 4097), (4097, 4097), (4097, 9001)):
        many.add(x[a:b])
    assert one.ntotal == many.ntotal == 9001
    D1, I1 = one.search(q, 20)
    D2, I2 = many.search(q, 20)
    assert np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def test_batch_invariance_and_run_to_run():
    """row r searched alone (the 32-row form of the kernel, another split of the database) is bitwise row r of a 259-row call (the
    128-row form), as is a 19-row slice; two calls agree"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(6)
    nx, nq = 20003, 259
    x = _rows(g, nx, 2048).to(DEV)
    xn = ops.row_sqnorm(x)
    q = (x[torch.randint(0, nx, (nq,), generator=g)].cpu() + _rows(g, nq, 2048, 0.5)).to(DEV)
    D, I = ops.flat_l2_topk(q, x, xn, 20)
    D2, I2 = ops.flat_l2_topk(q, x, xn, 20)
    assert torch.equal(I, I2) and torch.equal(D.view(torch.int32), D2.view(torch.int32))
    for r in (0, 31, 32, 127, 128, 258):
        Dr, Ir = ops.flat_l2_topk(q[r:r + 1], x, xn, 20)
        assert torch.equal(Ir[0], I[r]) and torch.equal(Dr[0].view(torch.int32), D[r].view(torch.int32)), r
    D19, I19 = ops.flat_l2_topk(q[100:119], x, xn, 20)
    assert torch.equal(I19, I[100:119]) and torch.equal(D19.view(torch.int32), D[100:119].view(torch.int32))


def test_row_sqnorm_vs_fp64():
    """16 lanes per row, each one fmaf chain over d / 16 squares, then a 4-step butterfly: every term is positive, so the relative
    error is at most (d / 16 + 4) 2^-24 (standard summation bound), 7.9e-6 at d = 2048"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(1)
    for d in (320, 2048):
        x = _rows(g, 1001, d, 3.0).to(DEV)
        ref = (x.double() ** 2).sum(1)
        tol = (d / 16 + 4) * 2.0 ** -24 * ref + 1e-12
        n = ops.row_sqnorm(x)
        assert ((n.double() - ref).abs() <= tol).all()
        idx = FlatL2Index(d, DEV)
        idx.add(x[:600])
        idx.add(x[600:].cpu().numpy())
        assert torch.equal(idx._norm[:1001], n)


def test_seq_scores_vs_fp64():
    """the pair table of test_search_gpu.test_seq_scores_vs_fp64 at d = 512. A lane adds n d / 64 products in one fmaf chain, six
    butterfly steps and a division follow: |error| <= (n d / 64 + 7) 2^-24 mean_i sum_c |q x| (standard summation bound)"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(8)
    nx, nq, d, k = 500, 40, 512, 6
    x = _rows(g, nx, d).to(DEV)
    q = _rows(g, nq, d).to(DEV)
    I = torch.randint(0, nx, (nq, k), generator=g)
    I[3, 2] = -1
    I[10, 0] = nx - 1                 # windows that run off the end of the index
    I[11, 5] = nx - 3
    I[20, :] = -1
    I = I.to(DEV)
    starts, lens = [0, 3, 10, 10, 20, 39], [5, 1, 11, 19, 2, 1]
    ldo = 19 * k
    out = ops.seq_scores(q, x, I, starts, lens, ldo).cpu().numpy()
    q64, x64, Ih = q.double().cpu().numpy(), x.double().cpu().numpy(), I.cpu().numpy()
    for p, (s, L) in enumerate(zip(starts, lens)):
        for j in range(ldo):
            cid = Ih[s + j // k, j % k] if j < L * k else -1
            if cid < 0:
                assert np.isnan(out[p, j])
                continue
            n = min(L, nx - cid)
            prod = q64[s:s + n] * x64[cid:cid + n]
            tol = (n * d / 64 + 7) * 2.0 ** -24 * np.abs(prod).sum() / n
            assert abs(out[p, j] - prod.sum() / n) <= tol, (p, j, out[p, j], prod.sum() / n, tol)


def test_launch_counters_and_refused_d():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import lib
    from neuralsampleid_amd.search import FlatL2Index
    xn = torch.zeros(64, device=DEV)
    ops.launch_counters(reset=True)
    y = torch.zeros(64, 2048, device=DEV)
    ops.flat_l2_topk(y, y, xn, 5)
    c = ops.launch_counters()
    assert c["flat_l2_topk"] == 1 and c["flat_l2_topk_wide"] == 1
    y = torch.zeros(64, 128, device=DEV)
    ops.flat_l2_topk(y, y, xn, 5)
    c = ops.launch_counters()
    assert c["flat_l2_topk"] == 2 and c["flat_l2_topk_wide"] == 1
    ops.launch_counters(reset=True)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    D = torch.empty(64, 5, device=DEV)
    I = torch.empty(64, 5, device=DEV, dtype=torch.int64)
    for d in (264, 288, 2112, 4096):
        y = torch.zeros(64, d, device=DEV)
        with pytest.raises(ValueError):
            ops.row_sqnorm(y)
        with pytest.raises(ValueError):
            ops.flat_l2_topk(y, y, xn, 5)
        with pytest.raises(ValueError):
            ops.seq_scores(y, y, I, [0], [1], 5)
        with pytest.raises(ValueError):
            FlatL2Index(d, DEV)
        assert lib.nsid_flat_l2_topk(y.data_ptr(), d, 64, y.data_ptr(), d, 64, xn.data_ptr(), xn.data_ptr(), d, 5, D.data_ptr(),
                                     I.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
        assert lib.nsid_row_sqnorm(y.data_ptr(), d, 64, d, xn.data_ptr(), None) == -1
    c = ops.launch_counters()
    assert c["row_sqnorm"] == c["flat_l2_topk"] == c["flat_l2_topk_wide"] == c["seq_scores"] == 0
