"""No GPU: the id mapping the GPU test of the leave-one-out search relies on against a brute-force deletion, the binding of
nsid_flat_l2_topk_excl, and the refusals of FlatL2Index.search(exclude=...) and of the leave_out keywords before any device call."""
import numpy as np
import pytest
import torch

from search_excl_oracle import brute_force, effective_range, groups, kept_rows, map_back


def test_id_mapping_equals_brute_force_deletion():
    """search the compacted database, map the ids back == delete the rows from the candidates of the full one"""
    rng = np.random.default_rng(0)
    nx, d, k = 23, 4, 6
    x = rng.integers(-2, 3, size=(nx, d)).astype(np.float64)          # small integers: exact distances, many ties
    x[9] = x[3]
    x[17] = x[3]
    q = x[[3, 3, 0, 5, 22, 11, 3, 8]] + 0.0
    ranges = [(0, 0), (3, 4), (0, 23), (4, 10), (22, 23), (2, 21), (0, 9), (-5, 2 ** 31 - 1)]
    lo, hi = [r[0] for r in ranges], [r[1] for r in ranges]
    D, I = brute_force(q, x, k, lo, hi)
    for i, (a, b) in enumerate(ranges):
        ea, eb = effective_range(a, b, nx)
        keep = kept_rows(a, b, nx)
        assert keep.size == nx - (eb - ea) and not ((keep >= ea) & (keep < eb)).any()
        Dc, Ic = brute_force(q[i:i + 1], x[keep], k, [0], [0])          # the plain search over what remains
        np.testing.assert_array_equal(map_back(Ic, ea, eb), I[i:i + 1])
        np.testing.assert_array_equal(Dc, D[i:i + 1])
        got = I[i][I[i] >= 0]
        assert not ((got >= ea) & (got < eb)).any() and got.size == min(k, keep.size)
    assert I[1].tolist()[:2] == [9, 17]                                 # the duplicates that remain, smaller id first
    assert I[6].tolist()[:2] == [9, 17] and I[0].tolist()[:3] == [3, 9, 17]
    assert (I[2] == -1).all() and np.isinf(D[2]).all() and (I[7] == -1).all()
    assert (I[5] >= 0).sum() == 4 and (I[5][4:] == -1).all()            # fewer than k rows remain: a padded tail
    assert map_back(np.array([-1, 0, 4, 5]), 4, 10).tolist() == [-1, 0, 10, 11]
    # grouping rows by their effective range: garbage and empty ranges fold onto (0, 0) or the clamped range
    g = dict((r, rows.tolist()) for r, rows in groups([0, 7, -5, 3, 9], [0, 7, 4, 1, 99], 23))
    assert g == {(0, 0): [0, 1, 3], (0, 4): [2], (9, 23): [4]}


def test_binding_and_limits():
    from neuralsampleid_amd import _lib, ops
    assert "nsid_flat_l2_topk_excl" in _lib.EXPORTS
    assert _lib.PROTOTYPES["nsid_flat_l2_topk_excl"] == ("i", "piipiippppiipppzs")
    assert _lib.PROTOTYPES["nsid_flat_l2_topk"] == ("i", "piipiippiipppzs")
    assert (ops.SEARCH_MAX_K, ops.VOTE_MAX_CAND) == (64, 4096)
    assert (ops.ALIGN_MAX_ROWS, ops.ALIGN_MAX_COLS, ops.ALIGN_MAX_TOP) == (4096, 4096, 64)
    keys = list(ops.launch_counters())
    assert keys[-2:] == ["flat_l2_topk_excl", "flat_l2_topk_wide_excl"]                # appended to the table
    # the C entry refuses bad shapes and null pointers without a device; nq = 0 is nothing to do
    N, einval = None, _lib.DEFINES["NSID_EINVAL"]
    before = ops.launch_counters()
    lib = _lib.lib
    assert lib.nsid_flat_l2_topk_excl(N, 128, 0, N, 128, 0, N, N, N, N, 128, 5, N, N, N, 0, N) == 0
    for d, k in ((120, 5), (272, 5), (2112, 5), (128, 0), (128, 65)):
        assert lib.nsid_flat_l2_topk_excl(N, d, 0, N, d, 0, N, N, N, N, d, k, N, N, N, 0, N) == einval, (d, k)
    assert lib.nsid_flat_l2_topk_excl(N, 128, 4, N, 128, 0, N, N, N, N, 128, 5, N, N, N, 0, N) == einval      # null pointers
    assert ops.launch_counters() == before


class _Recorder:
    """stands in for the ops a search would launch: records the calls, touches nothing"""

    def __init__(self):
        self.calls = []

    def plain(self, q, x, xn, k):
        self.calls.append(("plain", q.shape[0], None, None))
        return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64)

    def excl(self, q, x, xn, k, lo, hi):
        self.calls.append(("excl", q.shape[0], lo.tolist(), hi.tolist()))
        return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64)


def _host_index(monkeypatch, n=50, d=16):
    """a FlatL2Index object whose rows live on the host and whose ops are recorders: every refusal must come before them"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.search import FlatL2Index
    rec = _Recorder()
    monkeypatch.setattr(ops, "flat_l2_topk", rec.plain)
    monkeypatch.setattr(ops, "flat_l2_topk_excl", rec.excl)
    idx = FlatL2Index.__new__(FlatL2Index)
    idx.d, idx.device = d, torch.device("cpu")
    idx._x, idx._norm, idx._n = torch.zeros(n, d), torch.zeros(n), n
    return idx, rec


def test_search_exclude_is_checked_on_the_host(monkeypatch):
    from neuralsampleid_amd import search
    idx, rec = _host_index(monkeypatch)
    q = torch.zeros(6, 16)
    ok_lo, ok_hi = [0, 0, 10, 50, 49, 7], [0, 50, 20, 50, 50, 7]
    for bad in (([0] * 5, [0] * 5),                       # wrong length
                ([0] * 6, [0] * 7),
                ([0, 0, 21, 0, 0, 0], ok_hi),             # lo > hi
                (ok_lo, [0, 51, 20, 50, 50, 7]),          # hi > ntotal
                ([0, -1, 10, 50, 49, 7], ok_hi),          # negative lo
                ([0.5] * 6, [1.5] * 6),                   # not row ids
                (np.zeros((6, 1), np.int64), np.zeros((6, 1), np.int64)),
                [0] * 6, 5):                              # not a pair
        with pytest.raises(ValueError):
            idx.search(q, 3, exclude=bad)
    with pytest.raises(ValueError):
        idx.search(q, 65, exclude=(ok_lo, ok_hi))
    assert rec.calls == []
    # what passes is cut along with QUERY_BLOCK, and exclude=None makes the plain call
    monkeypatch.setattr(search, "QUERY_BLOCK", 4)
    idx.search(q, 3, exclude=(ok_lo, np.asarray(ok_hi)))
    assert rec.calls == [("excl", 4, ok_lo[:4], ok_hi[:4]), ("excl", 2, ok_lo[4:], ok_hi[4:])]
    rec.calls.clear()
    idx.search(q, 3)
    idx.search(q, 3, exclude=None)
    assert rec.calls == [("plain", 4, None, None), ("plain", 2, None, None)] * 2


def _host_sample_index(monkeypatch):
    """a SampleIndex of three songs (10, 20, 5 rows) after 7 dummy rows, on the host, with recorders for ops"""
    from neuralsampleid_amd import identify, ops
    from neuralsampleid_amd.identify import SampleIndex
    findex, rec = _host_index(monkeypatch, n=42, d=16)

    def touched(*a, **k):
        raise AssertionError("a device op was reached")
    for name in ("seq_scores", "song_vote", "pair_sim", "local_align", "row_sqnorm"):
        monkeypatch.setattr(ops, name, touched)
    monkeypatch.setattr(identify, "_need_cuda", lambda t, what: None)
    idx = SampleIndex(None, device="cuda")
    idx._index, idx._d, idx.n_dummy, idx.n_ref = findex, 16, 7, 35
    for code, (name, lo, n) in enumerate((("a", 0, 10), ("b", 10, 20), ("c", 30, 5))):
        idx.names.append(name)
        idx._code[name] = code
        idx._song_rows.append((lo, n, 0))
    return idx, rec


def test_leave_out_is_checked_before_the_device(monkeypatch):
    idx, rec = _host_sample_index(monkeypatch)
    fp = torch.zeros(12, 16)
    with pytest.raises(ValueError, match="different leave_out"):        # rows 4..5 are claimed for "a" and for "b"
        idx.identify_pairs(fp, [0, 4], [6, 6], leave_out=["a", "b"])
    with pytest.raises(ValueError, match="different leave_out"):        # a name and None conflict as well
        idx.identify_pairs(fp, [0, 5], [6, 6], leave_out=["a", None])
    with pytest.raises(ValueError, match="one song name"):
        idx.identify_pairs(fp, [0, 6], [6, 6], leave_out=["a"])
    with pytest.raises(KeyError):
        idx.identify_pairs(fp, [0], [6], leave_out=["no such song"])
    with pytest.raises(KeyError):
        idx.identify(fp=fp, leave_out="no such song")
    with pytest.raises(KeyError):
        idx.locate(fp=fp, threshold=0.5, leave_out="no such song")
    with pytest.raises(ValueError, match="songs="):
        idx.locate(fp=fp, threshold=0.5, songs=["a"], leave_out="b")
    with pytest.raises(ValueError, match="threshold"):
        idx.locate(fp=fp, leave_out="b")
    with pytest.raises(ValueError, match="threshold"):
        idx.links()
    with pytest.raises(KeyError):
        idx.links(names=["no such song"], threshold=0.5)
    with pytest.raises(TypeError):
        idx.links(names="a", threshold=0.5)
    with pytest.raises(ValueError):
        idx.links(names=["a", "a"], threshold=0.5)
    for kw in ({"k_probe": 65}, {"n_songs": 0}, {"top": 65}, {"block_rows": 0}, {"threshold": float("nan")}, {"row_hop_s": 0.5}):
        with pytest.raises(ValueError):
            idx.links(**{"threshold": 0.5, **kw})
    assert rec.calls == []
    # the ranges a valid call hands to the search: index ids (dummy ++ ref) of the song per row, (0, 0) where no pair names one
    lo, hi = idx._leave_out_ranges(["b", "b", None, "c"], np.array([0, 2, 6, 9]), np.array([4, 2, 3, 3]), 12)
    assert lo.tolist() == [17] * 4 + [0] * 5 + [37] * 3 and hi.tolist() == [37] * 4 + [0] * 5 + [42] * 3
    assert idx._leave_out_ranges([None, None], np.array([0, 2]), np.array([4, 2]), 12) is None
