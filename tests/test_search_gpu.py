"""GPU: exact flat-L2 search (csrc/search.hip) against fp64 brute force, its tie / batch / run-to-run invariants, the sequence
scores, and eval_hit_rates against the golden produced by the reference's own eval_faiss (tests/golden/make_search_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows(g, n, d, scale=1.0):
    return (torch.randn(n, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)).float()


def _fp64_dist(q, x, chunk=1 << 18):
    """(nq, nx) fp64 squared distances on the GPU, in database chunks"""
    q64 = q.to(DEV, torch.float64)
    qn = (q64 * q64).sum(1, keepdim=True)
    out = []
    for a in range(0, x.shape[0], chunk):
        x64 = x[a:a + chunk].to(DEV, torch.float64)
        out.append(qn + (x64 * x64).sum(1)[None, :] - 2.0 * q64 @ x64.T)
    return torch.cat(out, 1)


def _eps(q, x):
    """fp32 error bound of D: the f32-MFMA dot (<= ~1.5e-7 sum|q x| per the measured bound, taken x8) plus the norm roundings"""
    qn = q.double().norm(dim=1)
    xm = float(x.double().norm(dim=1).max()) if x.shape[0] else 0.0
    return (1.2e-6 * (qn * qn + xm * xm + 2 * qn * xm) + 1e-12).to(DEV)


def _check_topk(q, x, k, D, I):
    nq, nx = q.shape[0], x.shape[0]
    kk = min(k, nx)
    assert D.shape == (nq, k) and I.shape == (nq, k) and I.dtype == torch.int64
    if k > nx:
        assert (I[:, nx:] == -1).all() and torch.isinf(D[:, nx:]).all()
    if kk == 0:
        return
    Ik, Dk = I[:, :kk], D[:, :kk].double()
    assert (Ik >= 0).all() and (Ik < nx).all()
    assert (Dk[:, 1:] >= Dk[:, :-1]).all(), "D not ascending"
    for a in range(0, nq, 512):
        ref = _fp64_dist(q[a:a + 512], x)
        eps = _eps(q[a:a + 512], x)[:, None]
        got = ref.gather(1, Ik[a:a + 512])
        assert ((Dk[a:a + 512] - got).abs() <= eps).all(), float((Dk[a:a + 512] - got).abs().max())
        kth = ref.topk(kk, dim=1, largest=False).values[:, -1:]
        # every returned id lies within eps of the fp64 k-th; every id clearly inside the fp64 top-k is returned
        assert (got <= kth + 2 * eps).all()
        inside = ref < kth - 2 * eps
        hit = torch.zeros_like(inside)
        hit.scatter_(1, Ik[a:a + 512], True)
        assert not (inside & ~hit).any()
        assert ((Ik[a:a + 512].sort(1).values[:, 1:] != Ik[a:a + 512].sort(1).values[:, :-1])).all(), "duplicate ids"


CASES = [  # (nq, nx, d, k): every listed value of nq, nx, d and k at least once
    (1, 1, 64, 1),
    (19, 20, 128, 5),
    (128, 1000, 256, 20),
    (4099, 65537, 128, 64),
    (19, (1 << 20) + 3, 128, 20),
    (1, (1 << 20) + 3, 64, 64),
    (128, 1000, 64, 64),
]


@pytest.mark.parametrize("nq,nx,d,k", CASES)
def test_flat_l2_topk_vs_fp64(nq, nx, d, k):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(nq * 7 + nx + d + k)
    x = _rows(g, nx, d).to(DEV)
    q = (x[torch.randint(0, nx, (nq,), generator=g)].cpu() + _rows(g, nq, d, 0.3)).to(DEV)
    D, I = ops.flat_l2_topk(q, x, ops.row_sqnorm(x), k)
    torch.cuda.synchronize()
    _check_topk(q, x, k, D, I)


@pytest.mark.parametrize("nx,k", [(20, 64), (1, 5), (0, 3)])
def test_k_above_nx_pads(nx, k):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(5)
    x = _rows(g, nx, 128).to(DEV)
    q = _rows(g, 5, 128).to(DEV)
    D, I = ops.flat_l2_topk(q, x, ops.row_sqnorm(x), k)
    _check_topk(q, x, k, D, I)
    assert (I[:, nx:] == -1).all() and torch.isinf(D[:, nx:]).all() and (D[:, nx:] > 0).all()


def test_row_sqnorm_vs_fp64():
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(1)
    for d in (16, 128, 256):
        x = _rows(g, 1001, d, 3.0).to(DEV)
        n = ops.row_sqnorm(x)
        ref = (x.double() ** 2).sum(1)
        assert ((n.double() - ref).abs() <= 1e-6 * ref + 1e-12).all()


def test_exact_ties_and_self_match():
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(2)
    x = _rows(g, 5000, 128)
    x[100] = x[5]
    x[3000] = x[5]
    x[4999] = x[5]
    idx = FlatL2Index(128, DEV)
    idx.add(x.numpy())
    q = torch.stack([x[5] + 1e-3 * _rows(g, 1, 128)[0], x[17], x[4000]]).numpy()
    D, I = idx.search(q, 8)
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    assert list(I[0, :4]) == [5, 100, 3000, 4999]
    assert D[0, 0] == D[0, 1] == D[0, 2] == D[0, 3]
    assert I[1, 0] == 17 and I[2, 0] == 4000 and D[1, 0] < 1e-5 and D[2, 0] < 1e-5


def test_zero_rows():
    """rows zeroed by the NaN -> 0 load: a zero query ranks the zero database rows first, smaller id first, at distance 0"""
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(3)
    x = _rows(g, 3000, 128)
    zero = [7, 1234, 2999]
    x[zero] = 0.0
    idx = FlatL2Index(128, DEV)
    idx.add(x.to(DEV))
    D, I = idx.search(torch.zeros(2, 128, device=DEV), 5)
    assert I[:, :3].cpu().tolist() == [zero, zero] and (D[:, :3] == 0).all()
    assert (D[:, 3:] > 0).all()


def test_several_adds_equal_one():
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(4)
    x = _rows(g, 70001, 128).numpy()
    q = _rows(g, 300, 128).numpy()
    one = FlatL2Index(128, DEV)
    one.add(x)
    many = FlatL2Index(128, DEV)
    for a, b in ((0, 1), (1, 4097), (4097, 4097), (4097, 70001)):
        many.add(x[a:b])
    assert one.ntotal == many.ntotal == 70001
    D1, I1 = one.search(q, 20)
    D2, I2 = many.search(q, 20)
    assert np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def test_batch_invariance_and_run_to_run():
    """row r searched alone is bitwise row r of a 4099-row call (a different split of the database), and two calls agree"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(6)
    x = _rows(g, 200003, 128).to(DEV)
    xn = ops.row_sqnorm(x)
    q = (x[torch.randint(0, 200003, (4099,), generator=g)].cpu() + _rows(g, 4099, 128, 0.5)).to(DEV)
    D, I = ops.flat_l2_topk(q, x, xn, 20)
    D2, I2 = ops.flat_l2_topk(q, x, xn, 20)
    assert torch.equal(I, I2) and torch.equal(D.view(torch.int32), D2.view(torch.int32))
    for r in (0, 31, 32, 1000, 4098):
        Dr, Ir = ops.flat_l2_topk(q[r:r + 1], x, xn, 20)
        assert torch.equal(Ir[0], I[r]) and torch.equal(Dr[0].view(torch.int32), D[r].view(torch.int32)), r
    D19, I19 = ops.flat_l2_topk(q[1000:1019], x, xn, 20)
    assert torch.equal(I19, I[1000:1019]) and torch.equal(D19.view(torch.int32), D[1000:1019].view(torch.int32))


def test_seq_scores_vs_fp64():
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(8)
    nx, nq, d, k = 500, 40, 128, 6
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
            if j >= L * k:
                assert np.isnan(out[p, j])
                continue
            cid = Ih[s + j // k, j % k]
            if cid < 0:
                assert np.isnan(out[p, j])
                continue
            n = min(L, nx - cid)
            ref = np.mean(np.sum(q64[s:s + n] * x64[cid:cid + n], axis=1))
            assert abs(out[p, j] - ref) <= 1e-5, (p, j, out[p, j], ref)


def test_out_of_range_d_or_k_raises_without_launch():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    x = torch.zeros(64, 128, device=DEV)
    xn = torch.zeros(64, device=DEV)
    ops.launch_counters(reset=True)
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.flat_l2_topk(x, x, xn, k)
    for d in (8, 24, 272):
        y = torch.zeros(64, d, device=DEV)
        with pytest.raises(ValueError):
            ops.row_sqnorm(y)
        with pytest.raises(ValueError):
            ops.flat_l2_topk(y, y, xn, 5)
        with pytest.raises(ValueError):
            FlatL2Index(d, DEV)
    with pytest.raises(ValueError):
        FlatL2Index(128, DEV).search(np.zeros((2, 128), np.float32), 65)
    c = ops.launch_counters()
    assert c["row_sqnorm"] == c["flat_l2_topk"] == c["seq_scores"] == 0
    # the C entry points refuse them as well
    from neuralsampleid_amd._lib import lib
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    D = torch.empty(64, 65, device=DEV)
    I = torch.empty(64, 65, device=DEV, dtype=torch.int64)
    assert lib.nsid_flat_l2_topk(x.data_ptr(), 128, 64, x.data_ptr(), 128, 64, xn.data_ptr(), xn.data_ptr(), 128, 65, D.data_ptr(),
                                 I.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert lib.nsid_flat_l2_topk(x.data_ptr(), 128, 64, x.data_ptr(), 128, 64, xn.data_ptr(), xn.data_ptr(), 120, 5, D.data_ptr(),
                                 I.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert lib.nsid_row_sqnorm(x.data_ptr(), 128, 64, 272, xn.data_ptr(), None) == -1
    assert ops.launch_counters()["flat_l2_topk"] == 0


# ------------------------------------------------------------------------------------------------ the reference-made golden
def _file_digests(d):
    return {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))}


def test_eval_hit_rates_matches_reference_golden(tmp_path):
    from make_search_golden import load_golden_inputs, write_inputs
    from neuralsampleid_amd.search import FlatL2Index, eval_hit_rates
    z, inp = load_golden_inputs()
    emb = str(tmp_path / "emb")
    write_inputs(inp, emb)
    gt_path = str(tmp_path / "gt_dict.json")
    with open(gt_path, "w") as f:
        json.dump(inp["gt"], f)
    before = _file_digests(emb)
    params = json.loads(bytes(z["params"]).decode())
    hr = eval_hit_rates(emb, gt_path, test_seq_len=params["test_seq_len"], k_probe=params["k_probe"])
    after = _file_digests(emb)
    for f, h in before.items():
        assert after[f] == h, f"{f} was modified"
    assert set(after) - set(before) == {"hit_rates.npy", "raw_score.npy", "test_ids.npy"}
    np.testing.assert_array_equal(hr, z["hit_rates"])
    for name in ("hit_rates", "raw_score", "test_ids"):
        got = np.load(os.path.join(emb, name + ".npy"))
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])
    idx = FlatL2Index(inp["query"].shape[1], DEV)
    idx.add(inp["dummy"])
    idx.add(inp["ref"])
    _, I = idx.search(inp["query"], params["k_probe"])
    np.testing.assert_array_equal(I, z["I"].astype(np.int64))


def test_end_to_end_extraction_search(tmp_path):
    """ref DB from the product's extraction of synthetic clips; query DBs from a subset of the same clips under other names:
    every query is found top-1 at sl = 1"""
    from neuralsampleid_amd import fpdb
    from neuralsampleid_amd.search import eval_hit_rates
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    from synth import GRAFP_CFG, synth_clips, synth_state
    torch.manual_seed(0)
    model = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict(), ""))
    model = model.to(DEV).eval()
    x, _ = synth_clips(24)
    x = x.to(DEV)
    songs = [(f"song{i}", x[4 * i:4 * i + 4]) for i in range(6)]
    emb = str(tmp_path / "emb")
    fpdb.build_fp_db(model, songs, emb, "ref_db", batch=8)
    fpdb.build_fp_db(model, songs[:1], emb, "dummy_db", batch=8)
    queries = [(f"q{i}", x[4 * i + 1:4 * i + 3]) for i in (1, 3, 4)]
    fpdb.build_fp_db(model, queries, emb, "query_db", query_style=True, batch=8)
    gt = {f"song{i}": ([f"q{i}"] if i in (1, 3, 4) else []) for i in range(6)}
    # k_probe = 1: each query segment votes for the song of its nearest row only (with more probes the reference's summed score
    # lets a song with several near rows outvote the exact match: that is the metric, not the search)
    hr = eval_hit_rates(emb, gt, test_seq_len="1 2", k_probe=1, save=False)
    assert hr.shape == (3, 2) and hr[0, 0] == 100.0 and hr[0, 1] == 100.0, hr
