"""The rule of the certified bf16 pre-filter (include/nsid.h) restated on the CPU: bf16 through
tensor.bfloat16(), keys in fp64, E as derived. Nothing here is the code under test."""
import numpy as np
import torch

M = 64
PAD = 2 ** 31 - 1


def bf16(t: torch.Tensor) -> torch.Tensor:
    """the round-to-nearest-even bf16 image of fp32 rows, as fp32"""
    return t.float().bfloat16().float()


def stored_sqnorm(x: torch.Tensor) -> torch.Tensor:
    """a stored fp32 squared norm per row, as fp64 (the rule uses the same stored value in both keys, whatever its rounding)"""
    return (x.float() * x.float()).sum(1).double()


def exact_keys(q, x):
    return stored_sqnorm(x)[None, :] - 2.0 * (q.double() @ x.double().T)


def coarse_keys(q, x):
    return stored_sqnorm(x)[None, :] - 2.0 * (bf16(q).double() @ bf16(x).double().T)


def midpoint_rows(x: torch.Tensor) -> torch.Tensor:
    """every element moved just beside a bf16 rounding midpoint: the low 16 bits of the fp32 word become 0x7fff or 0x8001"""
    w = x.float().contiguous().view(torch.int32).clone()
    low = torch.where((torch.arange(w.numel()).reshape(w.shape) % 2) == 0, 0x7FFF, 0x8001).to(torch.int32)
    return ((w & ~0xFFFF) | low).view(torch.float32)


def bound(q, x):
    """E per query row (fp64) and its parts, from exact fp64 norms"""
    d = q.shape[1]
    qd, xd = q.double(), x.double()
    qb, xb = bf16(q).double(), bf16(x).double()
    eq = (qd - qb).norm(dim=1)
    Nq = torch.maximum(qd.norm(dim=1), qb.norm(dim=1))
    Xmax = torch.maximum(xd.norm(dim=1), xb.norm(dim=1)).max() if x.shape[0] else torch.tensor(0.0, dtype=torch.float64)
    EXmax = (xd - xb).norm(dim=1).max() if x.shape[0] else torch.tensor(0.0, dtype=torch.float64)
    slack = 2.0 ** -24 * (16.0 * d * Nq * Xmax + 8.0 * Xmax * Xmax) + 2.0 ** -100 * (1.0 + Nq + Xmax)
    return 2.0 * (eq * Xmax + Nq * EXmax) + slack, slack


def _order(key: np.ndarray, ids: np.ndarray) -> np.ndarray:
    return np.lexsort((ids, key))                   # by key, then id


def brute_topk(q, x, k, lo=None, hi=None):
    """fp64 brute force under (key, id) with excluded ranges: ids (nq, k) int64, -1 padded"""
    key = exact_keys(q, x).numpy()
    nq, nx = key.shape
    out = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        ids = np.arange(nx)
        if lo is not None:
            ids = ids[~((ids >= lo[i]) & (ids < hi[i]))]
        o = ids[_order(key[i, ids], ids)][:k]
        out[i, :o.size] = o
    return out


def certify(q, x, k, lo=None, hi=None):
    """the procedure of the rule: (ids (nq, k) int64 -1 padded, cert (nq,) bool, candidate ids per row)"""
    key, ckey = exact_keys(q, x).numpy(), coarse_keys(q, x).numpy()
    E = bound(q, x)[0].numpy()
    nq, nx = key.shape
    I = np.full((nq, k), -1, np.int64)
    cert = np.zeros(nq, bool)
    cands = []
    for i in range(nq):
        ids = np.arange(nx)
        if lo is not None:
            ids = ids[~((ids >= lo[i]) & (ids < hi[i]))]
        cand = ids[_order(ckey[i, ids], ids)][:M]
        cands.append(cand)
        top = cand[_order(key[i, cand], cand)][:k]
        I[i, :top.size] = top
        if cand.size < M:
            cert[i] = True                          # slot M - 1 is a pad: every competing row is a candidate
        else:
            thr = ckey[i, cand[M - 1]]
            cert[i] = bool(np.isfinite(E[i]) and thr - E[i] > key[i, top[k - 1]])
    return I, cert, cands
