"""No GPU: the retrieval hub case of the normalised candidate search in the fp32 oracles alone (the code under test is not involved),
the rule's edge cases in the oracle, the binding of nsid_flat_norm_topk, and the refusals of norm_search=True before any launch."""
import numpy as np
import pytest
import torch

import norm_search_oracle as ns
from diag_vote_oracle import diag_vote_pair
from locate_oracle import align_oracle


# ---------------------------------------------------------------------------------------------------- the rule in the oracle
def test_oracle_order_ties_nan_and_padding():
    z = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 0.0, -0.0, np.inf],
                  [np.nan] * 8], dtype=np.float32)
    Z, I = ns.norm_topk(z, 9)
    assert I[0].tolist() == [7, 1, 3, 0, 5, 6, 4, -1, -1]                    # equal z by id, +0 and -0 tie, NaN never
    assert Z[0][:7].tobytes() == z[0][[7, 1, 3, 0, 5, 6, 4]].tobytes() and np.isneginf(Z[0][7:]).all()
    assert (I[1] == -1).all() and np.isneginf(Z[1]).all()
    Z, I = ns.norm_topk(z, 3, lo=[1, 0], hi=[4, 0])                           # rows 1..3 do not compete for query row 0
    assert I[0].tolist() == [7, 0, 5] and (I[1] == -1).all()
    Z, I = ns.norm_topk(z, 2, lo=[5, 0], hi=[2, 0])                           # lo >= hi: nothing is left out
    assert I[0].tolist() == [7, 1]


# ---------------------------------------------------------------------------------------------------- the hub case
def test_hub_case_draws():
    dummy, songs, query = ns.hub_case(0)
    assert dummy.shape == (1024, 128) and len(songs) == 12 and all(s.shape == (64, 128) for s in songs) and query.shape == (48, 128)
    for t in [dummy, query] + songs:
        assert t.dtype == np.float32 and np.abs(np.linalg.norm(t.astype(np.float64), axis=1) - 1).max() < 1e-6
    again = ns.hub_case(0)
    assert np.array_equal(dummy, again[0]) and np.array_equal(query, again[2]) and all(np.array_equal(a, b) for a, b in zip(songs, again[1]))
    assert ns.default_cohort(dummy).shape == (512, 128) and np.array_equal(ns.default_cohort(dummy), dummy[::2])


@pytest.mark.parametrize("seed", list(ns.HUB_SEEDS))
def test_hub_case(seed):
    """k_probe = 20, one window of all 48 query rows. The L2 lists hold the true row (within one row) of none of the 32 planted query
    rows and the diagonal vote's first three songs exclude song 2; the normalised lists hold it for at least 30 of 32 and song 2 is
    first with at least twice the second song's count; the normalised alignment of song 2 at threshold 2.5, min_score 10 is exactly
    one occurrence within one row of (0, 31, 10, 41), and a hub song returns nothing."""
    h = ns.hub(seed)
    L, k = h["query"].shape[0], ns.HUB_K
    I_raw = ns.raw_topk(h["S"], h["x"], k)
    _, I_norm = ns.norm_topk(h["z"], k)
    raw = diag_vote_pair(I_raw, 0, L, h["song_of"], h["n_dummy"], top=5)
    nrm = diag_vote_pair(I_norm, 0, L, h["song_of"], h["n_dummy"], top=5)
    held_raw, _ = ns.planted_hits(I_raw, h)
    held, first = ns.planted_hits(I_norm, h)
    print(f"seed {seed}: raw lists hold the true row for {held_raw} of 32, raw vote {raw[0][:3]} {raw[1][:3]}; normalised lists hold "
          f"it for {held} (first for {first}), normalised vote {nrm[0][:3]} {nrm[1][:3]}")
    assert held_raw == 0 and 2 not in raw[0][:3]
    assert held >= 30 and nrm[0][0] == 2 and nrm[1][0] >= 2 * nrm[1][1]
    lo = h["n_dummy"] + int(h["song_start"][2])
    occ, _, n_occ, *_ = align_oracle(h["z"][:, lo:lo + 64], ns.HUB_THETA, ns.HUB_MIN_SCORE)
    assert n_occ == 1 and all(abs(int(occ[0][u]) - want) <= 1 for u, want in enumerate((0, 31, 10, 41))), (n_occ, occ[0])
    hub_song = raw[0][0]                                                     # the L2 vote's winner: a song with generic rows
    lo = h["n_dummy"] + int(h["song_start"][hub_song])
    assert hub_song in ns.HUB_GENERIC_SONGS and align_oracle(h["z"][:, lo:lo + 64], ns.HUB_THETA, ns.HUB_MIN_SCORE)[2] == 0


# ---------------------------------------------------------------------------------------------------- binding and refusals
def test_binding_counters_workspace_and_refusals_without_a_device():
    from neuralsampleid_amd import _lib, ops
    assert _lib.PROTOTYPES["nsid_flat_norm_topk"] == ("i", "piipiippppppiipppzs")
    assert {"flat_norm_topk", "flat_norm_topk_wide"} <= set(ops.launch_counters())
    lib, N, einval = _lib.lib, None, _lib.DEFINES["NSID_EINVAL"]
    for nq, nx in ((1, 100), (33, 5000), (130, 300), (8192, 262144)):
        assert lib.nsid_workspace_bytes(b"flat_norm_topk", nq, nx) == lib.nsid_workspace_bytes(b"flat_l2_topk", nq, nx) > 0
    before = ops.launch_counters()
    assert lib.nsid_flat_norm_topk(N, 128, 0, N, 128, 0, N, N, N, N, N, N, 128, 5, N, N, N, 0, N) == 0          # no row: nothing to do
    for d, k in ((120, 5), (272, 5), (2112, 5), (128, 0), (128, ops.SEARCH_MAX_K + 1)):
        assert lib.nsid_flat_norm_topk(N, d, 0, N, d, 0, N, N, N, N, N, N, d, k, N, N, N, 0, N) == einval, (d, k)
    assert lib.nsid_flat_norm_topk(N, 128, 4, N, 128, 0, N, N, N, N, N, N, 128, 5, N, N, N, 0, N) == einval      # null pointers
    assert ops.launch_counters() == before
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.flat_norm_topk(torch.zeros(4, 128), torch.zeros(64, 128), tuple(torch.zeros(n) for n in (4, 4, 64, 64)), 5)
    with pytest.raises(ValueError, match="outside"):
        ops.flat_norm_topk(torch.zeros(4, 128), torch.zeros(64, 128), None, 65)


class _Recorder:
    """stands in for the two searches of a FlatL2Index: records the call, touches nothing"""

    def __init__(self):
        self.calls = []

    def search(self, q, k, exclude=None, prefilter=None):
        self.calls.append("search")
        raise _Reached()

    def search_norm(self, q, k, norm, exclude=None):
        self.calls.append("search_norm")
        raise _Reached()


class _Reached(Exception):
    pass


def _host_sample_index(monkeypatch, prefilter=False):
    """a SampleIndex of three songs (10, 20, 5 rows) after 40 dummy rows whose state lives on the host: every refusal must come before
    an op, and the only thing a valid call reaches is the recorder"""
    from neuralsampleid_amd import identify, ops
    from neuralsampleid_amd.identify import SampleIndex

    def touched(*a, **k):
        raise AssertionError("a device op was reached")
    for name in ("seq_scores", "song_vote", "diag_vote", "pair_sim", "local_align", "row_sqnorm", "cohort_stats", "flat_norm_topk",
                 "flat_l2_topk", "flat_l2_topk_excl"):
        monkeypatch.setattr(ops, name, touched)
    monkeypatch.setattr(identify, "_need_cuda", lambda t, what: None)
    idx = SampleIndex(None, device="cuda", prefilter=prefilter)
    rec = _Recorder()
    rec.xb = torch.zeros(75, 16)
    idx._index, idx._d, idx.n_dummy, idx.n_ref = rec, 16, 40, 35
    for code, (name, lo, n) in enumerate((("a", 0, 10), ("b", 10, 20), ("c", 30, 5))):
        idx.names.append(name)
        idx._code[name] = code
        idx._song_rows.append((lo, n, 0))
    idx._cohort = torch.zeros(32, 16)
    return idx, rec


def test_norm_search_refusals_come_before_any_launch(monkeypatch):
    idx, rec = _host_sample_index(monkeypatch)
    fp = torch.zeros(12, 16)
    for call in (lambda **kw: idx.locate(fp=fp, threshold=2.5, **kw), lambda **kw: idx.scan(fp=fp, threshold=2.5, **kw),
                 lambda **kw: idx.scanner(threshold=2.5, **kw), lambda **kw: idx.links(threshold=2.5, **kw)):
        with pytest.raises(ValueError, match="vote='diagonal'"):
            call(norm_search=True)                                            # the default vote is the sequence vote
        with pytest.raises(ValueError, match="vote='diagonal'"):
            call(norm_search=True, vote="sequence")
    with pytest.raises(ValueError, match="rerank"):
        idx.locate(fp=fp, norm_search=True, rerank=True, vote="diagonal")
    with pytest.raises(ValueError, match="rerank"):
        idx.locate(fp=fp, norm_search=True, rerank=True)
    with pytest.raises(TypeError):                                            # no normalised sequence vote: the keyword does not exist
        idx.identify(fp=fp, norm_search=True)
    with pytest.raises(TypeError):
        idx.identify_pairs(fp, [0], [12], norm_search=True)
    pre, prec = _host_sample_index(monkeypatch, prefilter=True)
    for call in (lambda: pre.diag_votes(fp, [0], [12], norm_search=True),
                 lambda: pre.locate(fp=fp, threshold=2.5, vote="diagonal", norm_search=True),
                 lambda: pre.scanner(threshold=2.5, vote="diagonal", norm_search=True),
                 lambda: pre.links(threshold=2.5, vote="diagonal", norm_search=True)):
        with pytest.raises(ValueError, match="prefilter"):
            call()
    # the cohort refusals are normalize's: no cohort and too few dummy rows for a default one
    idx._cohort, idx.n_dummy = None, 7
    with pytest.raises(RuntimeError, match="cohort"):
        idx.diag_votes(fp, [0], [12], norm_search=True)
    with pytest.raises(RuntimeError, match="cohort"):
        idx.locate(fp=fp, threshold=2.5, vote="diagonal", norm_search=True)
    assert rec.calls == [] and prec.calls == []


def test_the_pre_filtered_index_refuses_search_norm():
    from neuralsampleid_amd.search import FlatL2Index
    idx = FlatL2Index.__new__(FlatL2Index)
    idx.d, idx.device, idx._n, idx._prefilter = 16, torch.device("cpu"), 50, True
    with pytest.raises(ValueError, match="pre-filter"):
        idx.search_norm(torch.zeros(3, 16), 5, tuple(torch.zeros(n) for n in (3, 3, 50, 50)))
    idx._prefilter = False
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match="outside"):
            idx.search_norm(torch.zeros(3, 16), bad_k, tuple(torch.zeros(n) for n in (3, 3, 50, 50)))
    with pytest.raises(ValueError, match="x_mu"):
        idx.search_norm(torch.zeros(3, 16), 5, tuple(torch.zeros(n) for n in (3, 3, 49, 50)))
    with pytest.raises(ValueError, match="norm must be"):
        idx.search_norm(torch.zeros(3, 16), 5, None)


def test_without_the_keyword_the_search_called_is_search(monkeypatch):
    idx, rec = _host_sample_index(monkeypatch)
    fp = torch.zeros(12, 16)
    with pytest.raises(_Reached):
        idx.diag_votes(fp, [0], [12])
    with pytest.raises(_Reached):
        idx.diag_votes(fp, [0], [12], norm_search=False)
    with pytest.raises(_Reached):
        idx.locate(fp=fp, threshold=2.5, vote="diagonal")
    assert rec.calls == ["search"] * 3
