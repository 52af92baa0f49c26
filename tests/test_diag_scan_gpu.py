"""GPU: the diagonal vote through SampleIndex: scan, scanner's trace, locate and links with vote="diagonal" on the synthetic catalogue
of diag_scan_case.py (whose expectations test_diag_vote_cpu.py proves for the rule on the host), and vote="sequence" spelled out
against the default call."""
import numpy as np
import pytest
import torch

import diag_scan_case as C
from diag_vote_oracle import diag_vote as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THETA, MIN_SCORE = 0.6, 2.0


@pytest.fixture(autouse=True)
def _fp32_switches():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module", params=C.RATES)
def scanned(request):
    """the catalogue in an index, the recording on the device, and one traced diagonal scan of it"""
    from neuralsampleid_amd.identify import SampleIndex
    rate = request.param
    songs, q = C.catalogue(rate)
    idx = SampleIndex(None, device=DEV)
    for s, rows in enumerate(songs):
        idx.add_rows(f"song {s}", _dev(rows))
    qd = _dev(q)
    sc = idx.scanner(threshold=THETA, min_score=MIN_SCORE, n_songs=1, vote="diagonal")
    sc.push(qd)
    occs = sc.finish()
    return rate, idx, qd, sc, occs


def _found(occs, names, plant, tol):
    want = C.plant_ends(plant)
    return [o for o in occs if o.song == names[plant[1]] and all(abs(g - w) <= tol for g, w in zip(o.q_rows + o.r_rows, want))]


def test_scan_finds_both_plants(scanned):
    rate, idx, qd, sc, occs = scanned
    inside, cross = C.plants(rate)
    assert len(_found(occs, idx.names, inside, 1 if rate == 1.0 else 2)) == 1, occs
    assert len(_found(occs, idx.names, cross, 1)) == 1, occs
    crossing = [o for o in occs if o.song == idx.names[cross[1]]]
    assert len(crossing) == 1 and crossing[0].q_rows[0] < C.WINDOW <= crossing[0].q_rows[1]          # found once, across the boundary
    assert idx.scan(fp=qd, threshold=THETA, min_score=MIN_SCORE, n_songs=1, vote="diagonal") == occs
    assert [t["start"] for t in sc.trace] == [0, C.WINDOW, 2 * C.WINDOW] and sc.window_rows == C.WINDOW


def test_trace_is_the_oracles_vote_on_the_same_search_result(scanned):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import DIAG_BIN_ROWS, DIAG_MIN_HITS
    rate, idx, qd, sc, _ = scanned
    song_of = idx._song_of[: idx.n_ref].cpu().numpy()
    inside, cross = C.plants(rate)
    for w, t in enumerate(sc.trace):
        rows = qd[w * C.WINDOW:(w + 1) * C.WINDOW].contiguous()
        _, I = idx._index.search(rows, C.K_PROBE)
        want = oracle(I.cpu().numpy(), [0], [C.WINDOW], song_of, idx.n_dummy, None, DIAG_BIN_ROWS, 1)
        keep = want[1][0] >= DIAG_MIN_HITS
        assert t["vote_codes"] == want[0][0][keep].tolist() and t["vote_totals"] == want[1][0][keep].tolist()
        first = idx._song_rows[t["vote_codes"][0]][0]
        assert t["vote_hints"] == [(w * C.WINDOW + int(want[2][0, 0]), w * C.WINDOW + int(want[3][0, 0]),
                                    int(want[4][0, 0]) - first, int(want[5][0, 0]) - first)]
    assert sc.trace[0]["vote_codes"] == [cross[1]] and sc.trace[1]["vote_codes"] == [inside[1]]
    assert sc.trace[1]["vote_totals"][0] >= inside[3]
    assert sc.trace[1]["active"] == [cross[1], inside[1]]              # the open path first, then the window's vote
    # the votes were diag_votes': one launch per window, no sequence scores
    before = ops.launch_counters()
    sc2 = idx.scanner(threshold=THETA, min_score=MIN_SCORE, n_songs=1, vote="diagonal")
    sc2.push(qd)
    sc2.finish()
    after = ops.launch_counters()
    assert after["diag_vote"] == before["diag_vote"] + 3
    assert after["seq_scores"] == before["seq_scores"] and after["song_vote"] == before["song_vote"]
    assert sc2.trace == sc.trace


def test_the_sequence_vote_misses_the_plant_inside_the_window(scanned):
    """what the diagonal vote is for: with the default vote and the same n_songs the plant inside window 1 is not a candidate"""
    rate, idx, qd, _, _ = scanned
    inside, _ = C.plants(rate)
    sc = idx.scanner(threshold=THETA, min_score=MIN_SCORE, n_songs=1)
    sc.push(qd)
    occs = sc.finish()
    assert sc.trace[1]["vote_codes"] != [inside[1]] and all(o.song != idx.names[inside[1]] for o in occs)
    assert all(t["vote_hints"] == [] for t in sc.trace)


def test_locate_and_diag_votes(scanned):
    rate, idx, qd, _, _ = scanned
    inside, _ = C.plants(rate)
    window = qd[C.WINDOW:2 * C.WINDOW]
    occs = idx.locate(fp=window, threshold=THETA, min_score=MIN_SCORE, vote="diagonal", n_songs=1)
    assert len(occs) == 1 and occs[0].song == idx.names[inside[1]]
    want = tuple(v - C.WINDOW if u < 2 else v for u, v in enumerate(C.plant_ends(inside)))
    assert all(abs(g - w) <= (1 if rate == 1.0 else 2) for g, w in zip(occs[0].q_rows + occs[0].r_rows, want))
    dv = idx.diag_votes(qd, [C.WINDOW, 0], [C.WINDOW, C.WINDOW], top=3)
    res = dv.results()
    assert len(dv) == 2 and res[0].songs[0] == idx.names[inside[1]] and res[0].counts[0] >= inside[3] and res[0].n_songs >= 3
    assert res[0].q_rows.shape == (3, 2) and res[0].q_rows[0, 0] <= inside[0] + 1 and res[0].q_rows[0, 1] >= inside[0] + inside[3] - 2
    excl = idx.diag_votes(qd, [C.WINDOW], [C.WINDOW], top=3, exclude=[idx.names[inside[1]]]).results()[0]
    assert idx.names[inside[1]] not in excl.songs and excl.n_songs == res[0].n_songs - 1
    assert len(idx.diag_votes(qd, [], [])) == 0


def test_sequence_spelled_out_is_the_default_call(scanned):
    from neuralsampleid_amd import ops
    _, idx, qd, _, _ = scanned
    kw = dict(threshold=THETA, min_score=MIN_SCORE)
    before = ops.launch_counters()["diag_vote"]
    assert idx.scan(fp=qd, **kw) == idx.scan(fp=qd, vote="sequence", **kw)
    assert idx.scan(fp=qd, n_songs=1, **kw) == idx.scan(fp=qd, n_songs=1, vote="sequence", bin_rows=4, min_hits=9, **kw)
    window = qd[C.WINDOW:2 * C.WINDOW]
    assert idx.locate(fp=window, **kw) == idx.locate(fp=window, vote="sequence", **kw)
    assert idx.locate(fp=qd[:300], n_songs=2, **kw) == idx.locate(fp=qd[:300], n_songs=2, vote="sequence", **kw)
    assert ops.launch_counters()["diag_vote"] == before                # the sequence path never takes the new kernel


def test_links_finds_a_sample_in_the_middle_of_a_long_song():
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.default_rng(31)
    a = C.unit_rows(rng, 64)
    b = C.unit_rows(rng, 300)
    b[130:170] = a[10:50]                                              # 40 rows of A in the middle of B
    idx = SampleIndex(None, device=DEV)
    for s in range(40):                                                # under the rule on the host: A's count in B's windows is 53, the next song's 27
        idx.add_rows(f"other {s}", _dev(C.unit_rows(rng, 64)))
    idx.add_rows("A", _dev(a))
    idx.add_rows("B", _dev(b))
    kw = dict(threshold=THETA, min_score=MIN_SCORE, n_songs=1)
    res = idx.links(vote="diagonal", **kw)
    in_b = [o for o in res.occurrences["B"] if o.song == "A"]
    assert len(in_b) == 1 and in_b[0].q_rows == (130, 169) and in_b[0].r_rows == (10, 49), res.occurrences["B"]
    assert [o.song for o in res.occurrences["A"]] == ["B"] and res.occurrences["A"][0].r_rows == (130, 169)
    lo, n, _ = idx._song_rows[idx.code("B")]
    assert res.occurrences["B"] == idx.locate(fp=idx.fingerprints[lo:lo + n], leave_out="B", vote="diagonal", **kw)
    assert idx.links(**kw).occurrences == idx.links(vote="sequence", **kw).occurrences
