"""No GPU: the rule of the certified bf16 pre-filter (tests/prefilter_oracle.py) is sound, the new entries are bound and refuse bad
arguments without a device, and FlatL2Index.search(prefilter=True) routes rows as the rule says (recorder ops)."""
import numpy as np
import pytest
import torch

import prefilter_oracle as po


def _inputs(kind, nq, nx, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nx, d, generator=g) / d ** 0.5
    q = x[torch.randint(0, nx, (nq,), generator=g)] + 0.3 * torch.randn(nq, d, generator=g) / d ** 0.5
    if kind == "positive":                          # the worst case of Cauchy-Schwarz: every product has the same sign
        x, q = x.abs(), q.abs()
    elif kind == "midpoint":                        # the largest bf16 rounding error in every element
        x, q = po.midpoint_rows(x), po.midpoint_rows(q)
    elif kind == "mixed":                           # row norms of 1e-3 .. 1e3
        x = x * (10.0 ** (6 * torch.rand(nx, 1, generator=g) - 3))
        q = q * (10.0 ** (6 * torch.rand(nq, 1, generator=g) - 3))
    return q.float(), x.float()


@pytest.mark.parametrize("d", [16, 128, 256, 2048])
@pytest.mark.parametrize("kind", ["random", "positive", "midpoint", "mixed"])
def test_bound_holds_for_every_pair(kind, d):
    q, x = _inputs(kind, 24, 300, d, d + len(kind))
    E, slack = po.bound(q, x)
    diff = (po.exact_keys(q, x) - po.coarse_keys(q, x)).abs()
    assert (diff <= E[:, None]).all(), float((diff - E[:, None]).max())
    assert (slack > 0).all()
    if kind == "random" and d <= 256:               # rows of one scale: the rounding slack is the small part of the bound
        assert (slack < 0.05 * E).all()
    if kind == "midpoint":                          # the rounding error really is near its maximum of 2^-9 per element
        rel = ((x.double() - po.bf16(x).double()).norm(dim=1) / x.double().norm(dim=1)).min()
        assert rel > 2.0 ** -9.6


@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", ["random", "positive", "midpoint", "mixed"])
def test_certified_rows_equal_brute_force(kind, d):
    q, x = _inputs(kind, 40, 900, d, 3 * d + len(kind))
    x[300], x[17] = x[512], x[512]                  # exact duplicates: equal keys, the smaller id first
    q[0] = x[512] + 1e-3 * q[0]
    q[1:8] = x[100:107] + 1e-5 * q[1:8]             # rows inside a tight cluster: more than M rows within E of each other
    x[600:720] = x[100] + 1e-5 * x[600:720]
    lo = np.array([(37 * i) % 800 for i in range(40)])
    hi = lo + np.array([0, 100] * 20)
    for k in (1, 20, 32):
        for ex in ((None, None), (lo, hi)):
            I, cert, _ = po.certify(q, x, k, *ex)
            want = po.brute_topk(q, x, k, *ex)
            assert cert.sum() >= 20 or kind == "mixed"                 # rows of very different norms share one Xmax: few or none certify
            np.testing.assert_array_equal(I[cert], want[cert])
    I, cert, _ = po.certify(q, x, 3)
    assert I[0].tolist() == [17, 300, 512] or not cert[0]
    assert cert[0] or kind == "mixed"
    # fewer than M competing rows: certified by the pad rule, padded tails
    I, cert, _ = po.certify(q[:4], x[:10], 20)
    assert cert.all() and (I[:, 10:] == -1).all() and (np.sort(I[:, :10], axis=1) == np.arange(10)).all()


def test_binding_and_refusals_without_a_device():
    from neuralsampleid_amd import _lib, ops
    assert _lib.PROTOTYPES["nsid_bf16_rows"] == ("i", "piiipipps")
    assert _lib.PROTOTYPES["nsid_flat_l2_topk_coarse"] == ("i", "piipiipppipppzs")
    assert _lib.PROTOTYPES["nsid_flat_l2_rescore"] == ("i", "piipiippppppppiipppps")
    for name in ("nsid_bf16_rows", "nsid_flat_l2_topk_coarse", "nsid_flat_l2_rescore"):
        assert name in _lib.EXPORTS
    assert (ops.PREFILTER_M, ops.PREFILTER_MAX_D) == (64, 256)
    keys = list(ops.launch_counters())
    assert {"bf16_rows", "flat_l2_topk_coarse", "flat_l2_rescore"} <= set(keys)
    lib, N, einval = _lib.lib, None, _lib.DEFINES["NSID_EINVAL"]
    assert lib.nsid_workspace_bytes(b"flat_l2_topk_coarse", 130, 4200) == 4 * 130 * 64 * 8
    assert lib.nsid_workspace_bytes(b"flat_l2_topk_coarse", 1, 100) == 64 * 8
    before = ops.launch_counters()
    # nothing to do
    assert lib.nsid_bf16_rows(N, 128, 0, 128, N, 128, N, N, N) == 0
    assert lib.nsid_flat_l2_topk_coarse(N, 128, 0, N, 128, 0, N, N, N, 128, N, N, N, 0, N) == 0
    assert lib.nsid_flat_l2_rescore(N, 128, 0, N, 128, 0, N, N, N, N, N, N, N, N, 128, 5, N, N, N, N, N) == 0
    # bad d, bad k, null pointers
    for d in (8, 120, 272, 320, 2048):
        assert lib.nsid_flat_l2_topk_coarse(N, d, 0, N, d, 0, N, N, N, d, N, N, N, 0, N) == einval, d
        assert lib.nsid_flat_l2_rescore(N, d, 0, N, d, 0, N, N, N, N, N, N, N, N, d, 5, N, N, N, N, N) == einval, d
    for d in (8, 120, 272, 2112):
        assert lib.nsid_bf16_rows(N, d, 0, d, N, d, N, N, N) == einval, d
    for k in (0, 65):
        assert lib.nsid_flat_l2_rescore(N, 128, 0, N, 128, 0, N, N, N, N, N, N, N, N, 128, k, N, N, N, N, N) == einval, k
    assert lib.nsid_bf16_rows(N, 128, 4, 128, N, 128, N, N, N) == einval
    assert lib.nsid_flat_l2_topk_coarse(N, 128, 4, N, 128, 0, N, N, N, 128, N, N, N, 0, N) == einval
    assert lib.nsid_flat_l2_rescore(N, 128, 4, N, 128, 0, N, N, N, N, N, N, N, N, 128, 5, N, N, N, N, N) == einval
    assert ops.launch_counters() == before


class _Recorder:
    """stands in for the ops a search would launch: records the calls, touches nothing"""

    def __init__(self, uncertified=()):
        self.calls = []
        self.uncertified = set(uncertified)         # row numbers of the whole call
        self.row0 = 0

    def plain(self, q, x, xn, k):
        self.calls.append(("plain", q[:, 0].tolist(), None, None))
        return torch.full((q.shape[0], k), 7.0), torch.full((q.shape[0], k), 7, dtype=torch.int64)

    def excl(self, q, x, xn, k, lo, hi):
        self.calls.append(("excl", q[:, 0].tolist(), lo.tolist(), hi.tolist()))
        return torch.full((q.shape[0], k), 7.0), torch.full((q.shape[0], k), 7, dtype=torch.int64)

    def pre(self, q, x, xb16, xn, xmax, exmax, k, ex=None):
        rows = q[:, 0].tolist()
        self.calls.append(("pre", rows, None if ex is None else ex[0].tolist(), None if ex is None else ex[1].tolist()))
        cert = torch.tensor([0 if int(r) in self.uncertified else 1 for r in rows], dtype=torch.uint8)
        return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64), cert


def _host_index(monkeypatch, d=16, n=50, uncertified=()):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    rec = _Recorder(uncertified)
    monkeypatch.setattr(ops, "flat_l2_topk", rec.plain)
    monkeypatch.setattr(ops, "flat_l2_topk_excl", rec.excl)
    monkeypatch.setattr(ops, "flat_l2_topk_pre", rec.pre)

    def touched(*a, **k):
        raise AssertionError("a device op was reached")
    for name in ("bf16_rows", "flat_l2_topk_coarse", "flat_l2_rescore", "row_sqnorm"):
        monkeypatch.setattr(ops, name, touched)
    idx = FlatL2Index.__new__(FlatL2Index)
    idx.d, idx.device = d, torch.device("cpu")
    idx._x, idx._norm, idx._n = torch.zeros(n, d), torch.zeros(n), n
    idx._prefilter, idx._nb16 = False, n
    idx._xb16 = torch.zeros(n, d, dtype=torch.bfloat16)
    idx._xmax = idx._exmax = torch.zeros(1)
    idx.prefilter_stats = {"rows": 0, "certified": 0, "fell_back": 0, "bypassed": 0}
    return idx, rec


def _queries(nq, d):
    q = torch.zeros(nq, d)
    q[:, 0] = torch.arange(nq)                      # a row carries its number: the recorders read it back
    return q


def test_prefilter_refusals_come_before_any_op(monkeypatch):
    idx, rec = _host_index(monkeypatch)
    q = _queries(6, 16)
    for kw in ({"k": 0}, {"k": 65}, {"exclude": ([0] * 5, [0] * 5)}, {"exclude": ([0, 0, 21, 0, 0, 0], [0, 50, 20, 50, 50, 7])},
               {"exclude": ([0] * 6, [51] * 6)}, {"exclude": 5}):
        with pytest.raises(ValueError):
            idx.search(q, **{"k": 3, "prefilter": True, **kw})
    with pytest.raises(ValueError):
        idx.search(torch.zeros(6, 32), 3, prefilter=True)
    assert rec.calls == [] and idx.prefilter_stats["rows"] == 0


def test_wide_rows_and_large_k_call_only_the_plain_op(monkeypatch):
    idx, rec = _host_index(monkeypatch, d=320)
    idx.search(_queries(3, 320), 5, prefilter=True)
    idx, rec2 = _host_index(monkeypatch, d=16)
    idx.search(_queries(3, 16), 33, prefilter=True)
    idx.search(_queries(3, 16), 33, exclude=([0, 1, 2], [5, 5, 5]), prefilter=True)
    assert [c[0] for c in rec.calls] == ["plain"] and [c[0] for c in rec2.calls] == ["plain", "excl"]
    assert idx.prefilter_stats == {"rows": 6, "certified": 0, "fell_back": 0, "bypassed": 6}
    idx.search(_queries(3, 16), 32, prefilter=True)                     # k = 32 is still served
    assert rec2.calls[-1][0] == "pre"
    idx._prefilter = True                                               # the index's own setting, and the keyword over it
    idx.search(_queries(2, 16), 5)
    idx.search(_queries(2, 16), 5, prefilter=False)
    assert [c[0] for c in rec2.calls[-2:]] == ["pre", "plain"]


def test_uncertified_rows_and_only_those_reach_the_plain_op(monkeypatch):
    from neuralsampleid_amd import search
    idx, rec = _host_index(monkeypatch, uncertified=(1, 4, 5, 9))
    monkeypatch.setattr(search, "QUERY_BLOCK", 4)
    q = _queries(10, 16)
    D, I = idx.search(q, 3, prefilter=True)
    assert rec.calls == [("pre", [0, 1, 2, 3], None, None), ("plain", [1], None, None),
                         ("pre", [4, 5, 6, 7], None, None), ("plain", [4, 5], None, None),
                         ("pre", [8, 9], None, None), ("plain", [9], None, None)]
    assert (I[:, 0] == 7).nonzero().flatten().tolist() == [1, 4, 5, 9] and (D[[1, 4, 5, 9]] == 7).all() and (D[[0, 2, 3]] == 0).all()
    assert idx.prefilter_stats == {"rows": 10, "certified": 6, "fell_back": 4, "bypassed": 0}
    rec.calls.clear()
    lo, hi = list(range(10)), [v + 20 for v in range(10)]
    idx.search(q, 3, exclude=(lo, hi), prefilter=True)
    assert rec.calls == [("pre", [0, 1, 2, 3], lo[:4], hi[:4]), ("excl", [1], [1], [21]),
                         ("pre", [4, 5, 6, 7], lo[4:8], hi[4:8]), ("excl", [4, 5], [4, 5], [24, 25]),
                         ("pre", [8, 9], lo[8:], hi[8:]), ("excl", [9], [9], [29])]
    rec.calls.clear()
    idx.search(q[:4], 3, prefilter=True)                                # nothing uncertified beyond row 1: one plain call of one row
    idx.search(q[2:4], 3, prefilter=True)
    assert [c[0] for c in rec.calls] == ["pre", "plain", "pre"]
