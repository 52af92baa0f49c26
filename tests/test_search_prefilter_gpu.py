"""GPU: the certified bf16 pre-filter (nsid_bf16_rows / nsid_flat_l2_topk_coarse / nsid_flat_l2_rescore, csrc/search.hip) against the
plain entries, bit for bit. The expected value is always ops.flat_l2_topk / ops.flat_l2_topk_excl, which tests/test_search_gpu.py pins
to the reference's golden; the kernels' own numbers are checked against fp64 on the host (tests/prefilter_oracle.py)."""
import json

import numpy as np
import pytest
import torch

import prefilter_oracle as po
from test_search_excl_gpu import _case, _i32, _rows, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_MAX = 2 ** 31 - 1
M = 64


class _Db:
    """what FlatL2Index keeps for the pre-filter, by hand: the rows, their norms, the bf16 copy and the two maxima"""

    def __init__(self, x):
        from neuralsampleid_amd import ops
        self.x = x.to(DEV).contiguous()
        self.xn = ops.row_sqnorm(self.x)
        self.xb, self.err, self.nrm = ops.bf16_rows(self.x)
        n = self.x.shape[0]
        self.xmax = self.nrm.max().reshape(1) if n else torch.zeros(1, device=DEV)
        self.exmax = self.err.max().reshape(1) if n else torch.zeros(1, device=DEV)

    def pre(self, q, k, ex=None):
        from neuralsampleid_amd import ops
        return ops.flat_l2_topk_pre(q, self.x, self.xb, self.xn, self.xmax, self.exmax, k, ex)

    def plain(self, q, k, ex=None):
        from neuralsampleid_amd import ops
        if ex is None:
            return ops.flat_l2_topk(q, self.x, self.xn, k)
        return ops.flat_l2_topk_excl(q, self.x, self.xn, k, ex[0], ex[1])


def _same_rows(got, want, rows):
    return _same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]))


def _near(g, x, nq, noise=0.3):
    d = x.shape[1]
    return x[torch.randint(0, x.shape[0], (nq,), generator=g)] + _rows(g, nq, d, noise)


@pytest.mark.parametrize("nx", [2100, 4200])               # 2 and 4 splits
@pytest.mark.parametrize("d", [16, 128, 256])
def test_certified_rows_equal_the_plain_search(d, nx):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(d + nx)
    db = _Db(_rows(g, nx, d))
    rows = certified = 0
    for nq in (1, 33, 65, 130):                            # a partial wave tile, two tiles, a partial 128-row block, two blocks
        q = _near(g, db.x.cpu(), nq).to(DEV)
        for k in (1, 20, 32):
            before = ops.launch_counters()
            D, I, cert = db.pre(q, k)
            after = ops.launch_counters()
            assert [after[c] - before[c] for c in ("bf16_rows", "flat_l2_topk_coarse", "flat_l2_rescore", "flat_l2_topk")] == [1, 1, 1, 0]
            ok = cert.bool()
            assert _same_rows((D, I), db.plain(q, k), ok), (nq, k)
            rows += nq
            certified += int(ok.sum())
    assert certified >= 0.9 * rows, (certified, rows)      # not a pass on fallback alone


def test_coarse_order_is_wrong_and_the_result_is_right():
    g = torch.Generator().manual_seed(5)
    d, nx = 128, 3000
    x = _rows(g, nx, d)
    q = _rows(g, 1, d)
    where = torch.randperm(nx, generator=g)[:30]
    x[where] = q + _rows(g, 30, d, 1e-4)
    order_exact = po.exact_keys(q, x[where])[0].argsort()
    order_coarse = po.coarse_keys(q, x[where])[0].argsort()
    assert not torch.equal(order_exact, order_coarse)
    db = _Db(x)
    D, I, cert = db.pre(q.to(DEV), 20)
    assert bool(cert[0]) and _same((D, I), db.plain(q.to(DEV), 20))
    assert set(I[0].tolist()) <= set(where.tolist())       # (their keys differ by ||noise||^2 ~ 1e-8: fp32 and fp64 order them differently)


def test_forced_fallback_inside_a_mixed_tile():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(8)
    d, nx, nq = 128, 3000, 40
    x = _rows(g, nx, d)
    q = _near(g, x, nq)
    hard = [3, 17, 35]
    for n, i in enumerate(hard):                           # 100 rows within 1e-4 of the query: more than M rows inside E of each other
        x[500 * (n + 1): 500 * (n + 1) + 100] = q[i] + _rows(g, 100, d, 1e-4)
    db = _Db(x)
    qd = q.to(DEV)
    D, I, cert = db.pre(qd, 20)
    assert (cert == 0).nonzero().flatten().tolist() == hard
    idx = FlatL2Index(d, DEV, prefilter=True)
    idx.add(x)
    before = ops.launch_counters()
    got = idx.search(qd, 20)
    after = ops.launch_counters()
    assert _same(got, db.plain(qd, 20))
    assert idx.prefilter_stats == {"rows": nq, "certified": nq - 3, "fell_back": 3, "bypassed": 0}
    assert (after["flat_l2_topk_coarse"] - before["flat_l2_topk_coarse"], after["flat_l2_topk"] - before["flat_l2_topk"]) == (1, 1)
    # k = 64 bypasses, and so does a wide index: the coarse counter does not move
    assert _same(idx.search(qd, 64), db.plain(qd, 64))
    for dw in (320, 2048):
        wide = FlatL2Index(dw, DEV, prefilter=True)
        xw = _rows(g, 300, dw)
        wide.add(xw)
        qw = xw[:5].to(DEV)
        assert _same(wide.search(qw, 5), ops.flat_l2_topk(qw, wide.xb, ops.row_sqnorm(wide.xb), 5))
        assert wide.prefilter_stats == {"rows": 5, "certified": 0, "fell_back": 0, "bypassed": 5} and wide._xb16 is None
    assert ops.launch_counters()["flat_l2_topk_coarse"] == after["flat_l2_topk_coarse"]
    assert idx.prefilter_stats["bypassed"] == nq
    # switched on later: the copy is built lazily, the keyword alone is enough
    late = FlatL2Index(d, DEV)
    late.add(x)
    assert late._xb16 is None and _same(late.search(qd, 20, prefilter=True), got) and late._nb16 == nx
    late.add(x[:10])
    late.enable_prefilter()
    assert late._nb16 == nx + 10 and late.prefilter_stats["fell_back"] == 3


def test_exact_ties_go_to_the_smaller_surviving_id():
    g = torch.Generator().manual_seed(2)
    d, nx = 128, 5000
    x = _rows(g, nx, d)
    dup = [5, 100, 1200, nx - 1]
    for j in dup[1:]:
        x[j] = x[5]
    q = torch.stack([x[5] + 1e-3 * _rows(g, 1, d)[0]] * 4).to(DEV)
    db = _Db(x)
    lo, hi = [0, 90, 0, 6], [0, 1201, 101, nx]
    ex = (_i32(lo), _i32(hi))
    D, I, cert = db.pre(q, 4, ex)
    assert cert.all() and _same((D, I), db.plain(q, 4, ex))
    assert I[0].tolist() == dup and I[1, :2].tolist() == [5, nx - 1] and I[2, :2].tolist() == [1200, nx - 1]
    D, I, cert = db.pre(q, 4)
    assert cert.all() and I[1].tolist() == dup and _same((D, I), db.plain(q, 4))


@pytest.mark.parametrize("nx,k", [(40, 20), (10, 20), (0, 5), (63, 32), (64, 32)])
def test_small_databases_are_certified_by_the_pad_rule(nx, k):
    g = torch.Generator().manual_seed(nx)
    db = _Db(_rows(g, nx, 128))
    q = _rows(g, 35, 128).to(DEV)
    D, I, cert = db.pre(q, k)
    assert _same((D, I), db.plain(q, k))
    if nx < M:
        assert cert.all() and (I[:, nx:] == -1).all() and torch.isinf(D[:, nx:]).all()


def test_leave_one_out_ranges_mixed_over_one_tile():
    nq, nx, d, k = 65, 2100, 128, 20
    q, x, lo, hi, planted = _case(nq, nx, d, k, 1088, 7)    # the twelve ranges of the leave-one-out tests, 1088 = the coarse split
    db = _Db(x)
    ex = (_i32(lo), _i32(hi))
    D, I, cert = db.pre(q, k, ex)
    want = db.plain(q, k, ex)
    ok = cert.bool()
    assert ok.sum() >= 0.9 * nq and _same_rows((D, I), want, ok) and planted
    In = I.cpu().numpy()
    for i in range(nq):
        real = In[i][In[i] >= 0]
        assert not ((real >= lo[i]) & (real < hi[i])).any(), i
    # garbage ranges are only ever compared
    kinds = [(-5, INT_MAX), (INT_MAX, -5), (-INT_MAX - 1, INT_MAX), (INT_MAX, INT_MAX), (-5, 50), (nx - 50, INT_MAX), (-INT_MAX - 1, -1),
             (7, 7)]
    ex = (_i32([kinds[i % 8][0] for i in range(nq)]), _i32([kinds[i % 8][1] for i in range(nq)]))
    D, I, cert = db.pre(q, k, ex)
    torch.cuda.synchronize()
    ok = cert.bool()
    assert ok.sum() >= 0.9 * nq and _same_rows((D, I), db.plain(q, k, ex), ok)
    assert all(bool(cert[i]) and (I[i] == -1).all() for i in range(nq) if i % 8 in (0, 2))       # nothing competes: the pad rule


@pytest.mark.parametrize("kind", ["random", "midpoint"])
def test_the_kernels_own_numbers(kind):
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(21)
    d, nx, nq = 128, 2100, 33
    x = _rows(g, nx, d)
    q = _near(g, x, nq)
    if kind == "midpoint":
        x, q = po.midpoint_rows(x), po.midpoint_rows(q)
    db = _Db(x)
    qd = q.to(DEV)
    # the bf16 image and the two norms
    assert torch.equal(db.xb.view(torch.int16), db.x.bfloat16().view(torch.int16))
    xd, xbd = x.double(), po.bf16(x).double()
    assert (db.err.cpu().double() >= (xd - xbd).norm(dim=1)).all() and (db.nrm.cpu().double() >= xd.norm(dim=1)).all()
    assert (db.nrm.cpu().double() >= xbd.norm(dim=1)).all()
    assert (db.err.cpu().double() <= (xd - xbd).norm(dim=1) * (1 + 1e-6)).all()            # rounded up, not blown up
    qb, q_err, q_nrm = ops.bf16_rows(qd)
    ckey, cid = ops.flat_l2_topk_coarse(qb, db.xb, db.xn)
    _, _, E, cert = ops.flat_l2_rescore(qd, db.x, db.xn, ops.row_sqnorm(qd), q_err, q_nrm, db.xmax, db.exmax, ckey, cid, 20)
    xn = db.xn.cpu().double()
    key = xn[None, :] - 2.0 * (q.double() @ xd.T)
    ck = xn[None, :] - 2.0 * (po.bf16(q).double() @ xbd.T)
    E_want, slack = po.bound(q, x)
    E, ckey, cid = E.cpu().double(), ckey.cpu().double(), cid.cpu().long()
    assert (E >= E_want).all() and (E <= E_want * 1.001).all()
    assert (cid >= 0).all() and (cid < nx).all() and all(cid[i].unique().numel() == M for i in range(nq))
    assert ((ckey - key.gather(1, cid)).abs() <= E[:, None]).all()
    assert ((ckey - ck.gather(1, cid)).abs() <= slack[:, None]).all()
    assert (ckey[:, 1:] >= ckey[:, :-1]).all()
    rest = torch.ones(nq, nx, dtype=torch.bool).scatter_(1, cid, False)
    assert (torch.where(rest, ck, torch.inf) >= (ckey[:, -1] - slack)[:, None]).all()
    if kind == "random":
        assert cert.all()


def test_batch_invariance_and_run_to_run():
    g = torch.Generator().manual_seed(6)
    nx, nq = 50003, 4099
    db = _Db(_rows(g, nx, 128))
    pick = torch.randint(0, nx, (nq,), generator=g)
    q = (db.x[pick].cpu() + _rows(g, nq, 128, 0.5)).to(DEV)
    a, b = db.pre(q, 20), db.pre(q, 20)
    assert _same(a[:2], b[:2]) and torch.equal(a[2], b[2]) and a[2].sum() >= 0.9 * nq
    assert _same_rows(a[:2], db.plain(q, 20), a[2].bool())
    for r in (0, 31, 32, 1000, 4098):
        one = db.pre(q[r:r + 1], 20)
        assert _same(one[:2], (a[0][r:r + 1], a[1][r:r + 1])) and int(one[2][0]) == int(a[2][r]), r


@pytest.mark.parametrize("what", ["nan query", "nan row", "huge row"])
def test_non_finite_inputs_are_never_certified_wrongly(what):
    from neuralsampleid_amd.search import FlatL2Index
    g = torch.Generator().manual_seed(31)
    d, nx, nq = 128, 2100, 40
    x = _rows(g, nx, d)
    q = _near(g, x, nq)
    if what == "nan query":
        q[5, 17] = float("nan")
    elif what == "nan row":
        x[700, 3] = float("nan")
    else:
        x[700] = 1e30
    db = _Db(x)
    qd = q.to(DEV)
    D, I, cert = db.pre(qd, 20)
    want = db.plain(qd, 20)
    ok = cert.bool()
    assert _same_rows((D, I), want, ok)
    if what == "nan query":
        assert not ok[5] and ok.sum() == nq - 1
    else:
        assert not ok.any()                                # the bound over the database is NaN or overflows: the plain search runs
    idx = FlatL2Index(d, DEV, prefilter=True)
    idx.add(x)
    assert _same(idx.search(qd, 20), want) and idx.prefilter_stats["fell_back"] == nq - int(ok.sum())


def test_eval_hit_rates_with_the_prefilter_matches_reference_golden(tmp_path):
    from make_search_golden import load_golden_inputs, write_inputs
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import eval_hit_rates
    z, inp = load_golden_inputs()
    emb = str(tmp_path / "emb")
    write_inputs(inp, emb)
    params = json.loads(bytes(z["params"]).decode())
    before = ops.launch_counters()
    hr = eval_hit_rates(emb, inp["gt"], test_seq_len=params["test_seq_len"], k_probe=params["k_probe"], prefilter=True)
    after = ops.launch_counters()
    assert after["flat_l2_topk_coarse"] > before["flat_l2_topk_coarse"]
    np.testing.assert_array_equal(hr, z["hit_rates"])
    for name in ("hit_rates", "raw_score", "test_ids"):
        got = np.load(f"{emb}/{name}.npy")
        assert got.dtype == z[name].dtype and got.shape == z[name].shape, name
        np.testing.assert_array_equal(got, z[name])


def test_sample_index_with_the_prefilter_returns_the_same_links_and_songs():
    from locate_oracle import PLANT_MIN_SCORE, PLANT_NOISE, PLANT_THETA, smooth_rows
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.Generator(np.random.PCG64(4))
    rows = [40, 90, 55, 70, 64, 81, 47, 60, 88, 52, 75, 43]
    songs = [smooth_rows(rng, n, 128) for n in rows]
    for s, a, r, b, n in ((0, 5, 3, 20, 30), (7, 10, 1, 40, 24)):          # two plants
        for t in range(n):
            v = songs[r][b + t] + PLANT_NOISE * rng.standard_normal(128) / np.sqrt(128)
            songs[s][a + t] = (v / np.linalg.norm(v)).astype(np.float32)
    dummy = smooth_rows(rng, 30, 128)
    out = []
    for pre in (False, True):
        idx = SampleIndex(None, device=DEV, prefilter=pre)
        idx.add_dummy(torch.from_numpy(dummy).to(DEV))
        for c, s in enumerate(songs):
            idx.add_rows(f"song {c:02d}", torch.from_numpy(s).to(DEV))
        before = ops.launch_counters()["flat_l2_topk_coarse"]
        res = idx.links(k_probe=20, n_songs=11, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16)
        ident = idx.identify(fp=torch.from_numpy(songs[0]).to(DEV), k_probe=20, top=10, leave_out="song 00")
        assert (ops.launch_counters()["flat_l2_topk_coarse"] > before) == pre
        if pre:
            assert idx._index.prefilter_stats["certified"] > 0
        occ = {n: [(o.song, o.q_rows, o.r_rows, np.float32(o.score).view(np.int32).item()) for o in v] for n, v in res.occurrences.items()}
        out.append((occ, ident.songs, ident.totals.view(np.int64).tolist()))
    assert out[0] == out[1] and any(out[0][0].values()) and out[0][1]


def test_bad_arguments_return_einval_and_launch_nothing():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import DEFINES, lib
    einval = DEFINES["NSID_EINVAL"]
    n, d = 64, 128
    x = torch.zeros(n, d, device=DEV)
    xb = torch.zeros(n, d, device=DEV, dtype=torch.bfloat16)
    f = torch.zeros(n, device=DEV)
    one = torch.zeros(1, device=DEV)
    z = torch.zeros(n, dtype=torch.int32, device=DEV)
    ck = torch.full((n, M), float("inf"), device=DEV)
    ci = torch.full((n, M), INT_MAX, device=DEV, dtype=torch.int32)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    D = torch.empty(n, 65, device=DEV)
    I = torch.empty(n, 65, device=DEV, dtype=torch.int64)
    cert = torch.empty(n, device=DEV, dtype=torch.uint8)
    Eb, Nb = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    ops.launch_counters(reset=True)
    P = lambda t: t.data_ptr()

    def rows(d=d, ldb=d, xp=P(x), bp=P(xb), ep=P(Eb)):
        return lib.nsid_bf16_rows(xp, d, n, d, bp, ldb, ep, P(Nb), None)

    def coarse(d=d, ld=d, qp=P(xb), lo=P(z), hi=P(z), kp=P(ck), wsb=ws.numel(), wsp=P(ws)):
        return lib.nsid_flat_l2_topk_coarse(qp, ld, n, P(xb), ld, n, P(f), lo, hi, d, kp, P(ci), wsp, wsb, None)

    def rescore(d=d, k=5, qp=P(x), xm=P(one), cp=P(ci), Ep=P(Eb), cert_p=P(cert)):
        return lib.nsid_flat_l2_rescore(qp, d, n, P(x), d, n, P(f), P(f), P(f), P(f), xm, P(one), P(ck), cp, d, k, P(D), P(I), Ep, cert_p, None)

    for kw in ({"d": 120}, {"d": 8}, {"d": 272}, {"ldb": 132}, {"ldb": 64}, {"xp": None}, {"bp": None}, {"ep": None}, {"bp": P(xb) + 2}):
        assert rows(**kw) == einval, kw
    for kw in ({"d": 120}, {"d": 8}, {"d": 272}, {"d": 320}, {"ld": 132}, {"qp": None}, {"lo": None}, {"hi": None}, {"kp": None},
               {"wsb": 16}, {"wsp": None}, {"qp": P(xb) + 2}):
        assert coarse(**kw) == einval, kw
    for kw in ({"d": 120}, {"d": 320}, {"k": 0}, {"k": 65}, {"qp": None}, {"xm": None}, {"cp": None}, {"Ep": None}, {"cert_p": None}):
        assert rescore(**kw) == einval, kw
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.flat_l2_rescore(x, x, f, f, f, f, one, one, ck, ci, k)
    with pytest.raises(ValueError):
        ops.flat_l2_topk_coarse(xb, xb, f, (z[:63], z))
    with pytest.raises(RuntimeError):
        ops.flat_l2_topk_coarse(x, xb, f)                  # fp32 rows where bf16 rows are expected
    wide = torch.zeros(8, 320, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.flat_l2_topk_coarse(wide, wide, f[:8])
    c = ops.launch_counters()
    assert c["bf16_rows"] == c["flat_l2_topk_coarse"] == c["flat_l2_rescore"] == c["flat_l2_topk"] == c["row_sqnorm"] == 0
    assert rows() == 0 and coarse() == 0 and coarse(lo=None, hi=None) == 0 and rescore() == 0
    c = ops.launch_counters()
    assert (c["bf16_rows"], c["flat_l2_topk_coarse"], c["flat_l2_rescore"]) == (1, 2, 1)
    torch.cuda.synchronize()
    assert not cert.any()                                  # 64 identical candidates (the coarse call's): no gap, no certificate
