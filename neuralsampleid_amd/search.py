"""Exact fingerprint search and song-level hit rates on the GPU (csrc/search.hip).

Reference: eval.py:198-367 `eval_faiss` with index_type='l2' (test_fp.py --small_test): a faiss.IndexFlatL2 over
dummy_db ++ ref_db, a top-k_probe search per query segment, the sequence score of every candidate and the song-level vote.
`FlatL2Index` stands in for the FAISS index and `eval_hit_rates` for the evaluation; both are written from the reference's
behaviour. One deliberate difference: the reference extends dummy_db.mm in place to hold dummy ++ ref (its fake_recon_index,
eval.py:263-267); here the database lives in GPU memory and every input file is left as it was.

    python -m neuralsampleid_amd.search --emb-dir DIR --gt gt_dict.json [--dummy-dir DIR] [--k-probe 20] [--test-seq-len "1 3 5"]
        [--prefilter]
"""
import argparse
import json
import os
import warnings
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import fpdb, ops

SLAB_BYTES = 256 << 20          # host -> device copies of a memmap in slabs of at most this size
QUERY_BLOCK = 65536             # query rows per flat_l2_topk launch (bounds the workspace)
PREFILTER_CUT_K = ops.PREFILTER_M // 2   # the pre-filter serves k up to here; larger k runs the plain search


class FlatL2Index:
    """faiss.IndexFlatL2 on the MI355X: exhaustive squared-L2 search, ids in add() order. search() of a numpy array returns
    numpy (float32 D, int64 I, as FAISS does); of a torch tensor, tensors on the index's device."""

    def __init__(self, d: int, device="cuda", prefilter: bool = False):
        """prefilter: search() runs the certified bf16 pre-filter (results are the plain search's bit for bit).
        The index then also keeps a bf16 copy of its rows (2 d more bytes per row) and two running maxima as device scalars."""
        d = int(d)
        if not ops.search_d_ok(d):
            raise ValueError(f"FlatL2Index: d = {d} is outside the search kernels' limits ({ops.SEARCH_D_LIMITS})")
        self.d = d
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FlatL2Index runs on the MI355X (cuda) device; there is no CPU path")
        self._x = torch.empty((0, d), device=self.device, dtype=torch.float32)
        self._norm = torch.empty((0,), device=self.device, dtype=torch.float32)
        self._n = 0
        self._prefilter = bool(prefilter)
        self._xb16 = None               # the bf16 rows, built by _sync_bf16 for the first _nb16 rows
        self._xmax = self._exmax = None  # device scalars >= max ||x_j|| (and of its bf16 image), >= max ||x_j - bf16(x_j)||
        self._nb16 = 0
        self.prefilter_stats = {"rows": 0, "certified": 0, "fell_back": 0, "bypassed": 0}

    @property
    def ntotal(self) -> int:
        return self._n

    @property
    def prefilter(self) -> bool:
        return self._prefilter

    def enable_prefilter(self) -> None:
        """switch the pre-filter on for later searches; the bf16 copy of the rows stored so far is built now"""
        self._prefilter = True
        self._sync_bf16()

    def _sync_bf16(self) -> None:
        """bring the bf16 copy and the running maxima up to the stored rows (nothing at a d the coarse kernel does not take)"""
        if not ops.prefilter_d_ok(self.d) or (self._xb16 is not None and self._nb16 == self._n):
            return
        if self._xb16 is None:
            self._xb16 = torch.empty((self._x.shape[0], self.d), device=self.device, dtype=torch.bfloat16)
            self._xmax = torch.zeros((1,), device=self.device, dtype=torch.float32)
            self._exmax = torch.zeros((1,), device=self.device, dtype=torch.float32)
            self._nb16 = 0
        if self._xb16.shape[0] < self._x.shape[0]:
            xb = torch.empty((self._x.shape[0], self.d), device=self.device, dtype=torch.bfloat16)
            xb[: self._nb16].copy_(self._xb16[: self._nb16])
            self._xb16 = xb
        step = max(1, SLAB_BYTES // (4 * self.d))
        for a in range(self._nb16, self._n, step):
            b = min(self._n, a + step)
            xb, err, nrm = ops.bf16_rows(self._x[a:b])
            self._xb16[a:b].copy_(xb)
            self._xmax = torch.maximum(self._xmax, nrm.max().reshape(1))       # NaN propagates: then no row is ever certified
            self._exmax = torch.maximum(self._exmax, err.max().reshape(1))
        self._nb16 = self._n

    @property
    def xb(self) -> torch.Tensor:
        """the stored rows (ntotal, d) on the device"""
        return self._x[: self._n]

    def _reserve(self, n: int) -> None:
        if n <= self._x.shape[0]:
            return
        cap = max(n, 2 * self._x.shape[0])
        x = torch.empty((cap, self.d), device=self.device, dtype=torch.float32)
        norm = torch.empty((cap,), device=self.device, dtype=torch.float32)
        x[: self._n].copy_(self._x[: self._n])
        norm[: self._n].copy_(self._norm[: self._n])
        self._x, self._norm = x, norm

    def add(self, x) -> None:
        """append rows: a numpy array / memmap (copied to the device in slabs of <= 256 MB) or a torch tensor"""
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"FlatL2Index.add: expected (n, {self.d}) rows, got {tuple(x.shape)}")
        n = int(x.shape[0])
        if self._n + n >= 2 ** 31:
            raise ValueError("FlatL2Index: row ids must stay below 2^31")
        self._reserve(self._n + n)
        step = max(1, SLAB_BYTES // (4 * self.d))
        for a in range(0, n, step):
            b = min(n, a + step)
            dst = self._x[self._n + a: self._n + b]
            if isinstance(x, torch.Tensor):
                dst.copy_(x[a:b])
            else:
                dst.copy_(torch.from_numpy(np.ascontiguousarray(x[a:b], dtype=np.float32)))
        if n:
            self._norm[self._n: self._n + n] = ops.row_sqnorm(self._x[self._n: self._n + n])
        self._n += n
        if self._prefilter:
            self._sync_bf16()

    def search(self, q, k: int, exclude=None, prefilter: Optional[bool] = None):
        """(nq, d) queries -> (D, I): (nq, k) squared L2 distances ascending and row ids; ties smaller id first; k > ntotal pads
        with I = -1, D = +inf. exclude = (lo, hi): two array-likes of nq row ids; the stored rows lo[i] <= j < hi[i] do not compete
        for query row i (leave-one-out search: the query is a run of stored rows), and its result is bitwise the search over the
        index without them. Checked on the host (0 <= lo <= hi <= ntotal) before the device is touched.
        prefilter (None: the index's setting): per QUERY_BLOCK the certified bf16 pre-filter (ops.flat_l2_topk_pre) runs first; the
        rows it does not certify are counted (one device-to-host read) and searched with the plain entry, so the result is the same
        bits either way. d > 256 and k > PREFILTER_M / 2 go straight to the plain entry. prefilter_stats counts the rows."""
        as_numpy = not isinstance(q, torch.Tensor)
        k = int(k)
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"FlatL2Index.search: k = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"FlatL2Index.search: expected (nq, {self.d}) queries, got {tuple(q.shape)}")
        ex = None if exclude is None else exclude_ranges(exclude, int(q.shape[0]), self._n)
        if as_numpy:
            qt = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(self.device)
        else:
            qt = q.to(device=self.device, dtype=torch.float32).contiguous()
        nq = qt.shape[0]
        D = torch.empty((nq, k), device=self.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
        if ex is not None:
            ex = torch.from_numpy(ex).to(self.device)           # one upload: rows 0 / 1 = lo / hi
        use = getattr(self, "_prefilter", False) if prefilter is None else bool(prefilter)     # (no setting: an index put together by hand)
        # k > M / 2 leaves fewer than M / 2 coarse keys between the k-th candidate and the threshold: the plain entry at once
        # (PREFILTER_CUT_K: a starting point, not yet moved by a measurement; docs/experiments.md)
        pre = use and ops.prefilter_d_ok(self.d) and k <= PREFILTER_CUT_K
        if pre:
            self._sync_bf16()
        norm = self._norm[: self._n]
        for a in range(0, nq, QUERY_BLOCK):
            b = min(nq, a + QUERY_BLOCK)
            exb = None if ex is None else (ex[0, a:b], ex[1, a:b])
            if pre:
                Db, Ib, cert = ops.flat_l2_topk_pre(qt[a:b], self.xb, self._xb16[: self._n], norm, self._xmax, self._exmax, k, exb)
                rest = torch.nonzero(cert == 0).flatten()                 # the one device-to-host read: how many rows remain
                if rest.numel():
                    qr = qt[a:b].index_select(0, rest)
                    if exb is None:
                        Dr, Ir = ops.flat_l2_topk(qr, self.xb, norm, k)
                    else:
                        Dr, Ir = ops.flat_l2_topk_excl(qr, self.xb, norm, k, exb[0].index_select(0, rest), exb[1].index_select(0, rest))
                    Db[rest], Ib[rest] = Dr, Ir
                D[a:b], I[a:b] = Db, Ib
                self.prefilter_stats["rows"] += b - a
                self.prefilter_stats["fell_back"] += int(rest.numel())
                self.prefilter_stats["certified"] += b - a - int(rest.numel())
                continue
            if use:
                self.prefilter_stats["rows"] += b - a
                self.prefilter_stats["bypassed"] += b - a
            if exb is None:
                D[a:b], I[a:b] = ops.flat_l2_topk(qt[a:b], self.xb, norm, k)
            else:
                D[a:b], I[a:b] = ops.flat_l2_topk_excl(qt[a:b], self.xb, norm, k, exb[0], exb[1])
        if as_numpy:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I

    def search_norm(self, q, k: int, norm, exclude=None):
        """(nq, d) device queries -> (Z, I): per row the k stored rows of largest cohort-normalised score (ops.flat_norm_topk: the
        cell ops.pair_sim(norm=) stores, bit for bit), Z (nq, k) descending and the row ids; equal scores smaller id first, a NaN score
        does not compete, and where fewer than k rows compete the tail is I = -1, Z = -inf. norm = (q_mu, q_rs, x_mu, x_rs): the
        cohort statistics of the rows of q and of ALL stored rows (ops.cohort_stats), device fp32. exclude: search's. The exact search
        itself is untouched; an index made with prefilter=True refuses (the certificate is a statement about L2 keys, and nothing
        like it has been derived for the normalised score)."""
        if getattr(self, "_prefilter", False):
            raise ValueError("FlatL2Index.search_norm: the bf16 pre-filter certifies L2 keys; there is no normalised pre-filter "
                             "(use an index made without prefilter=True)")
        k = int(k)
        if not 1 <= k <= ops.SEARCH_MAX_K:
            raise ValueError(f"FlatL2Index.search_norm: k = {k} is outside [1, {ops.SEARCH_MAX_K}]")
        if not isinstance(q, torch.Tensor) or q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"FlatL2Index.search_norm: expected (nq, {self.d}) device queries, got {tuple(getattr(q, 'shape', ()))}")
        if not isinstance(norm, (tuple, list)) or len(norm) != 4:
            raise ValueError("FlatL2Index.search_norm: norm must be (q_mu, q_rs, x_mu, x_rs)")
        nq = int(q.shape[0])
        for t, what, rows in zip(norm, ("q_mu", "q_rs", "x_mu", "x_rs"), (nq, nq, self._n, self._n)):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != rows:
                raise ValueError(f"FlatL2Index.search_norm: norm {what} must be a vector of {rows} entries")
        ex = None if exclude is None else exclude_ranges(exclude, nq, self._n)
        qt = q.to(device=self.device, dtype=torch.float32).contiguous()
        if ex is not None:
            ex = torch.from_numpy(ex).to(self.device)
        Z = torch.empty((nq, k), device=self.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
        q_mu, q_rs, x_mu, x_rs = norm
        for a in range(0, nq, QUERY_BLOCK):
            b = min(nq, a + QUERY_BLOCK)
            exb = None if ex is None else (ex[0, a:b], ex[1, a:b])
            Z[a:b], I[a:b] = ops.flat_norm_topk(qt[a:b], self.xb, (q_mu[a:b], q_rs[a:b], x_mu, x_rs), k, exb)
        return Z, I


def exclude_ranges(exclude, nq: int, ntotal: int) -> np.ndarray:
    """FlatL2Index.search's exclude = (lo, hi) checked on the host: a (2, nq) int32 array, or ValueError"""
    try:
        lo, hi = exclude
    except (TypeError, ValueError):
        raise ValueError("FlatL2Index.search: exclude must be a pair (lo, hi) of row-id sequences") from None
    lo, hi = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (lo, hi))
    if lo.ndim != 1 or hi.ndim != 1 or lo.size != nq or hi.size != nq:
        raise ValueError(f"FlatL2Index.search: exclude must hold one (lo, hi) per query row ({nq}), got {lo.shape} and {hi.shape}")
    if nq and not (np.issubdtype(lo.dtype, np.integer) and np.issubdtype(hi.dtype, np.integer)):
        raise ValueError("FlatL2Index.search: exclude must hold integer row ids")
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    if nq and (lo.min() < 0 or (lo > hi).any() or hi.max() > ntotal):
        raise ValueError(f"FlatL2Index.search: every excluded range needs 0 <= lo <= hi <= ntotal = {ntotal}")
    return np.stack([lo, hi]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ evaluation
def extract_test_ids(lookup: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """starts and lengths of the runs of equal strings in a query lookup table (eval.py:11-35), as int64 arrays"""
    if len(lookup) == 0:
        raise ValueError("extract_test_ids: the query lookup table is empty")
    a = np.asarray(lookup, dtype=object)
    change = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate([[0], change]).astype(np.int64)
    lens = np.diff(np.concatenate([starts, [len(a)]])).astype(np.int64)
    return starts, lens


def parse_seq_len(test_seq_len) -> np.ndarray:
    if isinstance(test_seq_len, str):
        test_seq_len = [int(v) for v in test_seq_len.split()]
    sl = np.asarray(test_seq_len, dtype=np.int64).reshape(-1)
    if sl.size == 0 or sl.min() < 1:
        raise ValueError(f"test_seq_len must hold positive lengths, got {test_seq_len!r}")
    return sl


def make_pairs(starts, lens, test_seq_len) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """the (test, sequence length) pairs the evaluation scores, test-major: (test index, length index, start row, length)"""
    starts, lens, sl = np.asarray(starts), np.asarray(lens), parse_seq_len(test_seq_len)
    ti, si = np.nonzero(sl[None, :] <= lens[:, None])
    return ti, si, starts[ti].astype(np.int64), sl[si].astype(np.int64)


def aggregate_hit_rates(I: np.ndarray, scores: np.ndarray, query_lookup: Sequence[str], ref_lookup: Sequence[str], n_dummy: int,
                        gt: Dict[str, Sequence[str]], test_seq_len='1 3 5 9 11 19'):
    """The song-level vote of eval.py:296-367 on the host, vectorised.

    I: (query rows, k) int64 ids over dummy ++ ref (-1 = none); scores: (pairs, >= max length * k) sequence scores of the
    candidates of make_pairs(...) in that order. Per pair the candidates are walked in the row-major order of its rows of I: ids
    below n_dummy and -1 are skipped, as is a ref song named like the query id (lookup.split('_')[0]); every remaining
    candidate adds its score to its song (duplicates again). Songs are ranked by descending score, ties in first-appearance
    order (Python's stable sorted(reverse=True)); top-1/3/10 = the query id is in gt[song] for one of the first 1 / 3 / 10. A
    song missing from gt counts as no hit. Returns (hit_rates (3, len(test_seq_len)) float64 in percent, raw_score
    (tests, 3 len(test_seq_len)) int64, test_ids = the tests' start rows, int64)."""
    I = np.asarray(I)
    scores = np.asarray(scores)
    if I.ndim != 2 or I.shape[0] != len(query_lookup):
        raise ValueError(f"aggregate_hit_rates: I must have one row per query segment ({len(query_lookup)}), got {I.shape}")
    n_dummy = int(n_dummy)
    if n_dummy < 0:
        raise ValueError("aggregate_hit_rates: n_dummy must be >= 0")
    sl = parse_seq_len(test_seq_len)
    starts, lens = extract_test_ids(query_lookup)
    ti, si, ps, pl = make_pairs(starts, lens, sl)
    k = I.shape[1]
    npairs = ti.size
    if scores.ndim != 2 or scores.shape[0] != npairs or (npairs and scores.shape[1] < int(pl.max()) * k):
        raise ValueError(f"aggregate_hit_rates: scores must be ({npairs}, >= {int(pl.max()) * k if npairs else 0}), got {scores.shape}")
    names, song_of = np.unique(np.asarray(ref_lookup, dtype=object).astype(str), return_inverse=True)
    code = {n: c for c, n in enumerate(names.tolist())}
    qid = [query_lookup[int(s)].split("_")[0] for s in starts]
    qcode = np.array([code.get(q, -1) for q in qid], dtype=np.int64)

    # every (pair, candidate) in walk order
    cnt = pl * k
    pair = np.repeat(np.arange(npairs), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    cid = I[ps[pair] + j // k, j % k] if pair.size else np.zeros(0, np.int64)
    keep = (cid >= 0) & (cid >= n_dummy) & (cid < n_dummy + len(ref_lookup))
    pair, j, cid = pair[keep], j[keep], cid[keep]
    song = song_of[cid - n_dummy]
    keep = song != qcode[ti[pair]]
    pair, j, song = pair[keep], j[keep], song[keep]
    val = scores[pair, j].astype(np.float64)

    # per (pair, song): summed score and first appearance (walk order = position in these arrays)
    key = pair.astype(np.int64) * len(names) + song
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if key.size else np.zeros(0, np.int64)
    total = np.add.reduceat(val, first) if key.size else np.zeros(0)
    gkey, gfirst = key[first], order[first]
    gpair, gsong = gkey // len(names), gkey % len(names)
    rank_order = np.lexsort((gfirst, -total, gpair))
    gpair, gsong = gpair[rank_order], gsong[rank_order]
    pstart = np.searchsorted(gpair, np.arange(npairs))
    rank = np.arange(gpair.size) - pstart[gpair] if gpair.size else np.zeros(0, np.int64)

    n_test, n_sl = starts.size, sl.size
    top = np.zeros((3, n_test, n_sl), dtype=np.int_)
    sel = np.flatnonzero(rank < 10)
    for e in sel.tolist():
        p = int(gpair[e])
        if qid[ti[p]] in gt.get(str(names[gsong[e]]), ()):
            r = int(rank[e])
            for m, lim in enumerate((1, 3, 10)):
                if r < lim:
                    top[m, ti[p], si[p]] = 1
    valid = sl[None, :] <= lens[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a length no test reaches: NaN, as the reference's nanmean gives
        hit_rates = np.stack([100.0 * np.nanmean(np.where(valid, top[m], np.nan), axis=0) for m in range(3)], axis=0)
    raw_score = np.concatenate((top[0], top[1], top[2]), axis=1)
    return hit_rates, raw_score, starts


def _load_gt(gt) -> Dict[str, Sequence[str]]:
    if isinstance(gt, (str, os.PathLike)):
        with open(gt) as f:
            gt = json.load(f)
    if not isinstance(gt, dict):
        raise TypeError("gt must be a dict {ref song: [query ids]} or the path of such a JSON file")
    return gt


def _open_rows(source_dir: str, fname: str):
    """a read-only memmap of a database file (fpdb's shape file and layout); NaN -> 0 happens on the copies in _slabs"""
    shape = fpdb.load_memmap_data(source_dir, fname, shape_only=True)
    return np.memmap(os.path.join(source_dir, fname + ".mm"), dtype="float32", mode="r", shape=(int(shape[0]), int(shape[1])))


def _slabs(mm, d):
    step = max(1, SLAB_BYTES // (4 * d))
    for a in range(0, mm.shape[0], step):
        s = np.array(mm[a:a + step], dtype=np.float32)
        s[np.isnan(s)] = 0.0                                          # eval.py load_memmap_data: NaN -> 0
        yield s


def _load_db(emb_dir, emb_dummy_dir, query_name, device, prefilter=False):
    """the databases of one evaluation: (FlatL2Index over dummy ++ ref, the query rows on its device, query lookup, ref lookup,
    rows of dummy_db). Shared by eval_hit_rates, rerank.py and baseline_eval.py."""
    query = _open_rows(emb_dir, query_name)
    ref = _open_rows(emb_dir, "ref_db")
    dummy = _open_rows(emb_dummy_dir, "dummy_db")
    d = query.shape[1]
    if ref.shape[1] != d or dummy.shape[1] != d:
        raise ValueError(f"dimension mismatch: query {query.shape}, ref {ref.shape}, dummy {dummy.shape}")
    query_lookup = fpdb.load_lookup(emb_dir, query_name)
    ref_lookup = fpdb.load_lookup(emb_dir, "ref_db")
    if len(query_lookup) != query.shape[0] or len(ref_lookup) != ref.shape[0]:
        raise ValueError("a lookup table does not have one entry per database row")
    index = FlatL2Index(d, device, prefilter=prefilter)
    for s in _slabs(dummy, d):                                        # index.add(dummy_db); index.add(db): eval.py:243-244
        index.add(s)
    for s in _slabs(ref, d):
        index.add(s)
    qt = torch.empty((query.shape[0], d), device=index.device, dtype=torch.float32)
    row = 0
    for s in _slabs(query, d):
        qt[row:row + s.shape[0]].copy_(torch.from_numpy(s))
        row += s.shape[0]
    return index, qt, query_lookup, ref_lookup, dummy.shape[0]


def eval_hit_rates(emb_dir: str, gt: Union[str, Dict[str, Sequence[str]]], emb_dummy_dir: Optional[str] = None,
                   test_seq_len='1 3 5 9 11 19', k_probe: int = 20, save: bool = True, device="cuda",
                   prefilter: bool = False):
    """eval.py eval_faiss(emb_dir, emb_dummy_dir, index_type='l2', test_seq_len=..., k_probe=...) on the GPU.

    Reads {query,ref}_db from emb_dir and dummy_db from emb_dummy_dir (default emb_dir) in fpdb's format; gt: {ref song:
    [query ids]} or its JSON path (the reference reads data/gt_dict.json). Returns hit_rates (3, len(test_seq_len)): top-1/3/10
    in percent per query length; with save, writes hit_rates.npy, raw_score.npy and test_ids.npy into emb_dir as the reference
    does. Input files are never modified. prefilter: the search runs through the certified bf16 pre-filter (same results)."""
    gt = _load_gt(gt)
    sl = parse_seq_len(test_seq_len)
    k_probe = int(k_probe)
    if not 1 <= k_probe <= ops.SEARCH_MAX_K:
        raise ValueError(f"k_probe = {k_probe} is outside [1, {ops.SEARCH_MAX_K}]")
    emb_dummy_dir = emb_dir if emb_dummy_dir is None else emb_dummy_dir
    index, qt, query_lookup, ref_lookup, n_dummy = _load_db(emb_dir, emb_dummy_dir, "query_db", device, prefilter)

    # every query row is searched once: a (test, length) pair uses rows [start, start + length) of the one result
    _, I = index.search(qt, k_probe)
    starts, lens = extract_test_ids(query_lookup)
    _, _, ps, pl = make_pairs(starts, lens, sl)
    scores = ops.seq_scores(qt, index.xb, I, ps, pl, int(sl.max()) * k_probe)
    hit_rates, raw_score, test_ids = aggregate_hit_rates(I.cpu().numpy(), scores.cpu().numpy(), query_lookup, ref_lookup,
                                                         n_dummy, gt, sl)
    if save:
        np.save(os.path.join(emb_dir, "hit_rates.npy"), hit_rates)
        np.save(os.path.join(emb_dir, "raw_score.npy"), raw_score)
        np.save(os.path.join(emb_dir, "test_ids.npy"), test_ids)
    return hit_rates


def format_hit_rates(hit_rates: np.ndarray, test_seq_len='1 3 5 9 11 19') -> str:
    sl = parse_seq_len(test_seq_len)
    lines = ["seq len " + "".join(f"{int(v):>8d}" for v in sl)]
    for name, row in zip(("top-1", "top-3", "top-10"), hit_rates):
        lines.append(f"{name:<8}" + "".join(f"{v:8.2f}" for v in row))
    return "\n".join(lines)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m neuralsampleid_amd.search", description=__doc__.split("\n\n")[0])
    ap.add_argument("--emb-dir", required=True, help="directory with query_db / ref_db (and dummy_db) in fpdb's format")
    ap.add_argument("--gt", required=True, help="JSON {ref song: [query ids]} (the reference's data/gt_dict.json)")
    ap.add_argument("--dummy-dir", default=None, help="directory of dummy_db (default: --emb-dir)")
    ap.add_argument("--k-probe", type=int, default=20)
    ap.add_argument("--test-seq-len", default="1 3 5 9 11 19")
    ap.add_argument("--no-save", action="store_true", help="do not write hit_rates.npy / raw_score.npy / test_ids.npy")
    ap.add_argument("--prefilter", action="store_true", help="search through the certified bf16 pre-filter (same results)")
    a = ap.parse_args(argv)
    hr = eval_hit_rates(a.emb_dir, a.gt, a.dummy_dir, a.test_seq_len, a.k_probe, save=not a.no_save, prefilter=a.prefilter)
    print(format_hit_rates(hr, a.test_seq_len))


if __name__ == "__main__":
    main()
