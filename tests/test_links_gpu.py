"""GPU: leave_out through SampleIndex (identify / identify_pairs / locate) and the catalogue self-join SampleIndex.links, on a synthetic
catalogue that needs no model: 12 songs of smooth rows after a few dummy rows, with plants between chosen pairs."""
import numpy as np
import pytest
import torch

from locate_oracle import PLANT_MIN_SCORE, PLANT_NOISE, PLANT_THETA, align_oracle, smooth_rows
from search_excl_oracle import map_back

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D_FP = 128
N_DUMMY = 40
SONG_ROWS = [300, 60, 180, 250, 90, 128, 275, 64, 200, 33 + 60, 150, 221]            # 12 songs of 60 .. 300 rows
# (song that samples, its first row, sampled song, its first row, rows, rate): song[a + t] = sampled[b + round(t rate)] + noise
PLANTS = [(0, 20, 3, 100, 40, 1.0), (2, 60, 6, 30, 24, 0.75), (5, 10, 8, 120, 12, 1.5), (10, 100, 1, 5, 30, 1.0)]
SEED = 1
# n_songs = 11: every other song that got a vote is aligned. The vote's sequence scores compare the query from its first row on, so a
# song that samples another in its middle gives its partner no better a total than chance; which songs share rows is for the alignment.
KW = dict(k_probe=20, n_songs=11, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.int32)


def _name(c):
    return f"song {c:02d}"


def make_catalogue(seed=SEED):
    """the songs' rows on the host: smooth rows, the plants written over them in locate_oracle.case's way"""
    rng = np.random.Generator(np.random.PCG64(seed))
    songs = [smooth_rows(rng, n, D_FP) for n in SONG_ROWS]
    for s, a, r, b, n, rate in PLANTS:
        for t in range(n):
            v = songs[r][b + int(round(t * rate))] + PLANT_NOISE * rng.standard_normal(D_FP) / np.sqrt(D_FP)
            songs[s][a + t] = (v / np.linalg.norm(v)).astype(np.float32)
    dummy = smooth_rows(rng, N_DUMMY, D_FP)
    return dummy, songs


def truth():
    """{song: [(partner, q rows (first, last), partner rows (first, last))]}, both directions of every plant"""
    out = {c: [] for c in range(len(SONG_ROWS))}
    for s, a, r, b, n, rate in PLANTS:
        last = b + int(round((n - 1) * rate))
        out[s].append((r, (a, a + n - 1), (b, last)))
        out[r].append((s, (b, last), (a, a + n - 1)))
    return out


def build_index(dummy, songs, names=None):
    from neuralsampleid_amd.identify import SampleIndex
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(dummy))
    for c, rows in enumerate(songs):
        idx.add_rows(_name(c) if names is None else names[c], _dev(rows))
    return idx


@pytest.fixture(scope="module")
def catalogue():
    dummy, songs = make_catalogue()
    idx = build_index(dummy, songs)
    assert idx.n_dummy == N_DUMMY > 0
    return idx, songs


def rows_of(idx, name):
    lo, n, _ = idx._song_rows[idx.code(name)]
    return idx.fingerprints[lo:lo + n]


def as_tuples(occs):
    return [(o.song, o.q_rows, o.r_rows, _bits(np.float32(o.score)).item(), o.q_time, o.r_time) for o in occs]


@pytest.fixture(scope="module")
def by_loop(catalogue):
    """what links must return: locate of every song's own rows with the song left out, computed once"""
    idx, songs = catalogue
    return {_name(c): idx.locate(fp=rows_of(idx, _name(c)), leave_out=_name(c), **KW) for c in range(len(songs))}


def matches(o, want):
    partner, q_rows, r_rows = want
    return o.song == _name(partner) and all(abs(g - w) <= 1 for g, w in zip(o.q_rows + o.r_rows, q_rows + r_rows))


# ------------------------------------------------------------------------------------------------ leave_out
def test_identify_pairs_with_leave_out_equals_the_pieces_by_hand(catalogue):
    from neuralsampleid_amd import ops
    idx, songs = catalogue
    for c in (0, 3, 9):
        name = _name(c)
        fp = rows_of(idx, name).contiguous()
        L = fp.shape[0]
        starts, lens = [0, 0, L - 50, 10], [L if L * 20 <= ops.VOTE_MAX_CAND else 100, 30, 50, 1]
        pv = idx.identify_pairs(fp, starts, lens, k_probe=20, top=10, leave_out=[name] * 4)
        lo = idx.n_dummy + idx._song_rows[c][0]
        hi = lo + L
        xb, xn = idx._index.xb, ops.row_sqnorm(idx._index.xb)
        _, Ic = ops.flat_l2_topk(fp, torch.cat([xb[:lo], xb[hi:]]).contiguous(), torch.cat([xn[:lo], xn[hi:]]).contiguous(), 20)
        Ih = map_back(Ic.cpu().numpy(), lo, hi)
        assert not ((Ih >= lo) & (Ih < hi)).any() and (Ih >= 0).all()
        I = torch.from_numpy(Ih).to(DEV)
        scores = ops.seq_scores(fp, xb, I, starts, lens, max(lens) * 20)
        codes, totals, n = ops.song_vote(I, scores, starts, lens, idx._song_of[: idx.n_ref], idx.n_dummy, None, 10)
        assert torch.equal(pv.codes, codes) and torch.equal(pv.totals.view(torch.int64), totals.view(torch.int64))
        assert torch.equal(pv.n_songs, n) and not (pv.codes == c).any() and (pv.n_songs > 0).all()
        # one pair through identify
        m = min(L, 100)
        r = idx.identify(fp=fp[:m].contiguous(), k_probe=20, top=10, leave_out=name)
        one = idx.identify_pairs(fp[:m].contiguous(), [0], [m], k_probe=20, top=10, leave_out=[name]).results()[0]
        assert r.songs == one.songs and name not in r.songs and np.array_equal(r.totals.view(np.int64), one.totals.view(np.int64))


def _mixed_pair(seed):
    """a song that plays another one under its own material (rows = own + sampled, normalised): every row's nearest rows are its own
    song's, as with real overlapping segments; (dummy, [sampler, sampled, others...])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    songs = [smooth_rows(rng, n, D_FP) for n in (40, 120, 80, 100, 70)]
    v = songs[0] + songs[1][30:70]
    songs[0] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return smooth_rows(rng, 10, D_FP), songs


def test_leave_out_finds_what_exclude_floods():
    for seed in range(20):                                            # the first seed whose fp64 distance table shows the flooding
        dummy, songs = _mixed_pair(seed)
        table = np.concatenate([dummy] + songs).astype(np.float64)
        a = table[10:50]
        dist = (a * a).sum(1)[:, None] + (table * table).sum(1)[None, :] - 2.0 * a @ table.T
        near = np.argsort(dist, axis=1, kind="stable")[:, :3]
        if ((near >= 10) & (near < 50)).all():
            break
    else:
        raise AssertionError("no seed shows the flooding")
    idx = build_index(dummy, songs)
    fp = rows_of(idx, _name(0))
    flooded = idx.identify(fp=fp, exclude=_name(0), k_probe=3)
    assert _name(1) not in flooded.songs and flooded.n_songs == 0       # its own rows took every slot, the vote threw them away
    found = idx.identify(fp=fp, leave_out=_name(0), k_probe=3)
    assert found.songs[0] == _name(1) and _name(0) not in found.songs
    # locate: the same query finds where
    occs = idx.locate(fp=fp, leave_out=_name(0), k_probe=3, threshold=0.5, min_score=2.0)
    assert occs and occs[0].song == _name(1) and abs(occs[0].r_rows[0] - 30) <= 1 and abs(occs[0].r_rows[1] - 69) <= 1
    assert idx.locate(fp=fp, exclude=_name(0), k_probe=3, threshold=0.5, min_score=2.0) == []


# ------------------------------------------------------------------------------------------------ links
@pytest.mark.parametrize("block_rows", [700, 1 << 16])
def test_links_equals_the_loop_of_locate(catalogue, by_loop, block_rows):
    idx, songs = catalogue
    if block_rows == 700:                                             # three or more blocks
        sizes, used = 1, 0
        for n in SONG_ROWS:
            if used and used + n > 700:
                sizes, used = sizes + 1, 0
            used += n
        assert sizes >= 3
    res = idx.links(block_rows=block_rows, **KW)
    assert res.skipped == [] and list(res.occurrences) == [_name(c) for c in range(len(songs))]
    for name, occs in res.occurrences.items():
        assert as_tuples(occs) == as_tuples(by_loop[name]), name
    # a subset, out of add order (the query rows are gathered), with a row timing
    names = [_name(6), _name(0), _name(3)]
    sub = idx.links(names=names, row_hop_s=0.5, row_len_s=1.0, block_rows=block_rows, **KW)
    assert list(sub.occurrences) == names
    for name in names:
        want = idx.locate(fp=rows_of(idx, name), leave_out=name, row_hop_s=0.5, row_len_s=1.0, **KW)
        assert as_tuples(sub.occurrences[name]) == as_tuples(want) and want[0].q_time is not None
    # a small score budget cuts the pairs into chunks and changes nothing
    tight = idx.links(s_budget_bytes=4 * 300 * 300, block_rows=block_rows, **KW)
    assert {n: as_tuples(o) for n, o in tight.occurrences.items()} == {n: as_tuples(o) for n, o in res.occurrences.items()}


def test_links_reports_every_plant_in_both_directions(catalogue, by_loop):
    idx, songs = catalogue
    res = idx.links(**KW)
    want = truth()
    assert sum(len(v) for v in want.values()) == 2 * len(PLANTS) and sum(1 for v in want.values() if not v) >= 4
    for c, plants in want.items():
        occs = res.occurrences[_name(c)]
        assert len(occs) == len(plants), (c, occs)
        for p in plants:
            assert sum(matches(o, p) for o in occs) == 1, (c, p, occs)
    # the host oracle on fp64 score matrices says the same of EVERY pair of songs: the plants and nothing else
    for c in range(len(songs)):
        for o in range(len(songs)):
            if o == c:
                continue
            S = (songs[c].astype(np.float64) @ songs[o].astype(np.float64).T).astype(np.float32)
            occ, _, n_occ, *_ = align_oracle(S, PLANT_THETA, PLANT_MIN_SCORE, 16)
            here = [p for p in want[c] if p[0] == o]
            assert n_occ == len(here), (c, o, occ[:n_occ].tolist())
            for p in here:
                assert sum(all(abs(g - w) <= 1 for g, w in zip(row, p[1] + p[2])) for row in occ[:n_occ].tolist()) == 1


LINK_KEYS = ("flat_l2_topk", "flat_l2_topk_wide", "flat_l2_topk_excl", "flat_l2_topk_wide_excl", "seq_scores", "song_vote", "pair_sim",
             "local_align", "row_sqnorm")


def _launches(idx):
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    res = idx.links(**KW)
    after = ops.launch_counters()
    return res, {k: after[k] - before[k] for k in LINK_KEYS}


def test_links_launches_do_not_grow_with_the_songs(catalogue):
    idx, songs = catalogue
    res, n12 = _launches(idx)
    one_block = {"flat_l2_topk": 0, "flat_l2_topk_wide": 0, "flat_l2_topk_excl": 1, "flat_l2_topk_wide_excl": 0, "seq_scores": 1,
                 "song_vote": 1, "pair_sim": 1, "local_align": 1, "row_sqnorm": 1}
    assert n12 == one_block
    halves, names = [], []
    for c, rows in enumerate(songs):                                  # the same rows registered as 24 songs
        m = rows.shape[0] // 2
        halves += [rows[:m], rows[m:]]
        names += [f"{_name(c)} a", f"{_name(c)} b"]
    dummy, _ = make_catalogue()
    idx24 = build_index(dummy, halves, names)
    assert torch.equal(idx24._index.xb, idx._index.xb) and len(idx24.names) == 24
    res24, n24 = _launches(idx24)
    assert n24 == one_block and len(res24.occurrences) == 24
    assert sum(len(v) for v in res24.occurrences.values()) >= 2 * len(PLANTS)


def test_links_skips_a_song_past_the_row_limit(catalogue):
    idx, songs = catalogue
    kw = {**KW, "n_songs": 12}                                        # room for every song that votes, with the long one among them
    base = idx.links(**kw)
    dummy, _ = make_catalogue()
    rng = np.random.Generator(np.random.PCG64(99))
    big = build_index(dummy, songs + [smooth_rows(rng, 4097, D_FP)])
    res = big.links(**kw)
    assert res.skipped == [_name(12)] and _name(12) not in res.occurrences and len(res.occurrences) == 12
    for name, occs in base.occurrences.items():
        assert as_tuples(res.occurrences[name]) == as_tuples(occs), name
        assert all(o.song != _name(12) for o in res.occurrences[name])
    only = big.links(names=[_name(12), _name(1)], **kw)
    assert only.skipped == [_name(12)] and list(only.occurrences) == [_name(1)]


def test_refusals_launch_nothing(catalogue):
    from neuralsampleid_amd import ops
    idx, songs = catalogue
    fp = rows_of(idx, _name(1))
    before = ops.launch_counters()
    with pytest.raises(ValueError, match="threshold"):
        idx.links()
    with pytest.raises(KeyError):
        idx.links(names=["no such song"], threshold=0.6)
    with pytest.raises(KeyError):
        idx.identify(fp=fp, leave_out="no such song")
    with pytest.raises(KeyError):
        idx.locate(fp=fp, threshold=0.6, leave_out="no such song")
    with pytest.raises(ValueError, match="songs="):
        idx.locate(fp=fp, threshold=0.6, songs=[_name(2)], leave_out=_name(1))
    with pytest.raises(ValueError, match="different leave_out"):
        idx.identify_pairs(fp, [0, 10], [20, 20], leave_out=[_name(1), _name(2)])
    assert ops.launch_counters() == before
