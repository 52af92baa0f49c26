"""GPU: local_align_strip chained against the cell loop of the whole matrix bit for bit, a path at the length bound, align_occurrences
against the oracle, and SampleIndex.scanner / scan: the streaming form of align, the voted scan with its active-set rule, a recording
past 4096 rows, the cap on the active songs, and every refusal."""
import numpy as np
import pytest
import torch

from locate_oracle import PLANT_MIN_SCORE, PLANT_NOISE, PLANT_THETA, align_cells, case, dyadic, smooth_rows
from scan_oracle import align_chained, occurrences_unpacked, replay_active, rows_from_cells

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345


@pytest.fixture(autouse=True)
def _fp32_switches():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ local_align_strip
# (Lq, Lr): 1030 and 4096 columns need the 1024-thread workgroup and more than one column per thread, 257 two columns of 256 threads
STRIP_PAIRS = [(150, 1), (150, 2), (150, 3), (150, 64), (150, 65), (150, 257), (150, 1030), (24, 4096)]
ROW_BASES = [0, 32760, 65530, 2 ** 30]
# per cut: the strips of the 150-row pairs and of the 24-row pair (the shorter list is filled up with strips of 0 rows)
STRIP_CUTS = {"whole": ((150,), (24,)), "ones": ((1,) * 150, (1,) * 24), "2-0-1": ((2, 0, 1, 143, 4), (2, 0, 1, 17, 4)),
              "last-alone": ((149, 1), (23, 1)), "64s": ((64, 64, 22), (10, 10, 4))}


@pytest.fixture(scope="module")
def strip_cases():
    """per pair: (S, H, org) of the cell loop on the whole matrix, computed once"""
    rng = np.random.default_rng(77)
    out = []
    for Lq, Lr in STRIP_PAIRS:
        S = dyadic(rng, Lq, Lr)
        H, org = align_cells(S, 0.5)
        out.append((S, H, org, rows_from_cells(S, 0.5, H, org, 0)))
    return out


def _open_after(H, done):
    """the largest H in the last two of the first `done` rows"""
    m = np.float32(0)
    for r in (done - 1, done - 2):
        if r >= 0 and H.shape[1]:
            m = max(m, H[r].max())
    return np.float32(m)


def _run_chain(ops, cases, which, cuts150, cuts24, rot):
    """the pairs `which` through one launch per strip: odd pairs start one launch late (so fresh and continuing pairs share a launch),
    a pair's row_base is ROW_BASES[(pair + rot) % 4]. Returns per pair (rows, carry, open_h per launch) and the row buffers."""
    P = len(which)
    mats = [cases[p][0] for p in which]
    q_tot = [m.shape[0] for m in mats]
    x_len = np.asarray([m.shape[1] for m in mats], dtype=np.int64)
    base = [ROW_BASES[(p + rot) % 4] for p in which]
    cuts = []
    for n, (p, m) in enumerate(zip(which, mats)):
        c = list(cuts150 if m.shape[0] == 150 else cuts24)
        cuts.append([0] * (n % 2) + c)
    launches = max(len(c) for c in cuts)
    cuts = [c + [0] * (launches - len(c)) for c in cuts]
    s_size = np.asarray([m.size for m in mats], dtype=np.int64)
    s_base = np.cumsum(s_size) - s_size
    S = _dev(np.concatenate([m.reshape(-1) for m in mats]))
    carry, carry_off = ops.align_carry(x_len, DEV)
    gap = 8                                                           # sentinel cells between the pairs' rows; a strip of 0 rows points there
    r_base = np.cumsum([q + gap for q in q_tot]) - np.asarray(q_tot) - gap + gap
    total = int(sum(q_tot) + gap * (P + 1))
    rows = (torch.full((total,), float(SENTINEL), device=DEV), torch.full((total,), SENTINEL, device=DEV, dtype=torch.int32),
            torch.full((total,), SENTINEL, device=DEV, dtype=torch.int32), torch.full((total,), SENTINEL, device=DEV, dtype=torch.int32))
    done = [0] * P
    started = [False] * P
    opens = []
    before = ops.launch_counters()["local_align_strip"]
    for t in range(launches):
        q_len = np.asarray([c[t] for c in cuts], dtype=np.int64)
        fresh = [0 if started[n] else 1 for n in range(P)]
        s_off = s_base + np.asarray(done) * x_len
        row_off = [int(r_base[n]) + done[n] if q_len[n] else int(r_base[n]) - gap for n in range(P)]
        res = ops.local_align_strip(S, s_off, x_len, q_len, x_len, 0.5, [base[n] + done[n] for n in range(P)], fresh, carry, carry_off,
                                    rows=rows, row_off=row_off)
        assert res[0] is rows[0] and res[4].tolist() == row_off
        opens.append(res[5])
        for n in range(P):
            done[n] += int(q_len[n])
            started[n] = started[n] or q_len[n] > 0
    assert ops.launch_counters()["local_align_strip"] == before + launches           # every pair of a strip in one launch
    assert done == q_tot
    return rows, r_base, carry, carry_off, torch.stack(opens).cpu().numpy(), cuts, base, gap


def _check_chain(ops, cases, which, cuts150, cuts24, rot):
    got = _run_chain(ops, cases, which, cuts150, cuts24, rot)
    rows, r_base, carry, carry_off, opens, cuts, base, gap = got
    host = [t.cpu().numpy() for t in rows]
    ch, ci, cj = (t.cpu().numpy() for t in carry)
    covered = np.zeros(host[0].size, dtype=bool)
    for n, p in enumerate(which):
        S, H, org, want = cases[p]
        Lq, Lr = S.shape
        a, b = int(r_base[n]), int(r_base[n]) + Lq
        covered[a:b] = True
        msg = f"pair {p} {S.shape} row_base {base[n]}"
        np.testing.assert_array_equal(_bits(host[0][a:b]), _bits(want[0]), err_msg=msg)
        np.testing.assert_array_equal(host[1][a:b], want[1], err_msg=msg)
        np.testing.assert_array_equal(host[2][a:b], np.where(want[2] >= 0, want[2] + base[n], -1), err_msg=msg)
        np.testing.assert_array_equal(host[3][a:b], want[3], err_msg=msg)
        done = 0
        for t, c in enumerate(cuts[n]):
            done += c
            assert _bits(opens[t, n]) == _bits(_open_after(H, done)), (msg, t)
        co = int(carry_off[n])
        for r in (0, 1):                                               # the carry holds the last two rows of the whole matrix
            i = Lq - 1 - r
            sl = slice(co + r * Lr, co + (r + 1) * Lr)
            np.testing.assert_array_equal(_bits(ch[sl]), _bits(H[i]), err_msg=msg)
            np.testing.assert_array_equal(ci[sl], np.where(org[i] >= 0, (org[i] >> 16) + base[n], -1), err_msg=msg)
            np.testing.assert_array_equal(cj[sl], np.where(org[i] >= 0, org[i] & 0xffff, -1), err_msg=msg)
    for u in range(4):                                                 # nothing else was written: the strips of 0 rows point at the gaps
        assert (host[u][~covered] == SENTINEL).all()
    again = _run_chain(ops, cases, which, cuts150, cuts24, rot)       # the same bits a second time
    for u in range(4):
        assert torch.equal(again[0][u].view(torch.int32), rows[u].view(torch.int32))
    assert np.array_equal(_bits(again[4]), _bits(opens))
    for u in range(3):
        assert torch.equal(again[2][u].view(torch.int32), carry[u].view(torch.int32))


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("cut", list(STRIP_CUTS))
def test_chained_strips_equal_the_cell_loop_bit_for_bit(strip_cases, cut, rot):
    from neuralsampleid_amd import ops
    _check_chain(ops, strip_cases, list(range(len(STRIP_PAIRS))), *STRIP_CUTS[cut], rot)


@pytest.mark.parametrize("cut", ["ones", "2-0-1", "64s"])
def test_small_pairs_alone_take_the_narrow_workgroup(strip_cases, cut):
    """up to 1024 columns the launch has 256 threads; the results do not depend on it"""
    from neuralsampleid_amd import ops
    cuts150, cuts24 = STRIP_CUTS[cut]
    _check_chain(ops, strip_cases, [0, 1, 2, 3, 4, 5], cuts150, cuts24, 1)


def test_strip_cases_hold_paths_ties_and_long_origins(strip_cases):
    """what the comparison above stands on: paths that cross every cut, exact ties, origins many rows back"""
    S, H, org, want = strip_cases[6]
    assert (want[2] >= 0).sum() > 100 and (strip_cases[0][3][2] == -1).any()     # and rows without a passing cell at Lr = 1
    hv = H[H > 0]
    assert hv.size > np.unique(hv).size
    back = (np.arange(150) - want[2])[want[2] >= 0]
    assert back.max() >= 8                                             # a path longer than any strip of the "ones" and "2-0-1" cuts


@pytest.mark.parametrize("row_base", [0, 32600])
def test_a_path_at_the_length_bound_keeps_its_origin(row_base):
    """one path of (2, 1) steps over all 300 columns: i - i0 = 598 at its end, in strips of 7 rows; with row_base = 32600 the origin row
    and the rows of the path lie on both sides of 2^15"""
    from neuralsampleid_amd import ops
    Lr, Lq = 300, 599
    S = np.zeros((Lq, Lr), dtype=np.float32)
    for t in range(Lr):
        S[2 * t, t] = 1.0
    cuts = [7] * (Lq // 7) + [Lq % 7]
    want = align_chained(S, 0.5, cuts, row_base)
    Sd = _dev(S.reshape(-1))
    carry, carry_off = ops.align_carry([Lr], DEV)
    parts, lo = [], 0
    for n in cuts:
        res = ops.local_align_strip(Sd, [lo * Lr], [Lr], [n], [Lr], 0.5, [row_base + lo], [1 if lo == 0 else 0], carry, carry_off)
        parts.append([t.cpu().numpy() for t in res[:4]])
        assert float(res[5][0]) > 0                                    # the path is open at every cut
        lo += n
    got = [np.concatenate([p[u] for p in parts]) for u in range(4)]
    on = np.arange(0, Lq, 2)
    assert (got[2][on] == row_base).all() and (got[3][on] == 0).all()  # the origin survives every strip
    assert (got[1][on] == np.arange(Lr)).all()
    assert (got[0][on] == 0.5 * (np.arange(Lr) + 1)).all()
    assert int((on[-1] + row_base) - got[2][on[-1]]) == 598
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    for u in (1, 2, 3):
        np.testing.assert_array_equal(got[u], want[u])


def test_pairs_without_columns_and_pairs_past_the_host_maxima():
    """x_len = 0: empty rows and open_h = 0. A pair whose device lengths exceed the host maxima (the C entry called directly: ops never
    passes such a pair) reads nothing, writes its rows as empty, leaves its carry and gets open_h = -1; its neighbour is not disturbed"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import call
    rng = np.random.default_rng(8)
    S = dyadic(rng, 6, 9)
    want = align_chained(S, 0.5, (6,), 40)
    Sd = _dev(S.reshape(-1))
    carry, carry_off = ops.align_carry([0, 9], DEV)
    rh, rj, ri, rc, row_off, oh = ops.local_align_strip(Sd, [0, 0], [1, 9], [5, 6], [0, 9], 0.5, [7, 40], [1, 1], carry, carry_off)
    rh, rj, ri, rc, oh = (t.cpu().numpy() for t in (rh, rj, ri, rc, oh))
    assert row_off.tolist() == [0, 5] and (rh[:5] == 0).all() and (rj[:5] == -1).all() and (ri[:5] == -1).all() and (rc[:5] == -1).all()
    np.testing.assert_array_equal(_bits(rh[5:]), _bits(want[0]))
    np.testing.assert_array_equal(ri[5:], want[2])
    assert oh[0] == 0 and _bits(oh[1]) == _bits(want[5][-1])
    # device lengths past the host maxima: pair 0 says 6 x 9 where the host said at most 4 rows; pair 1 is in order (4 rows)
    p = lambda t: t.data_ptr()
    i32 = _dev(np.asarray([[9, 9], [6, 4], [9, 9], [40, 40], [1, 1]], dtype=np.int32))        # s_ld, q_len, x_len, row_base, fresh
    i64 = _dev(np.asarray([[0, 0], [0, 18], [0, 6]], dtype=np.int64))                         # s_off, carry_off, row_off
    ch = torch.full((36,), 7.0, device=DEV)
    ci, cj = (torch.full((36,), 7, device=DEV, dtype=torch.int32) for _ in range(2))
    rows = (torch.full((10,), float(SENTINEL), device=DEV),) + tuple(torch.full((10,), SENTINEL, device=DEV, dtype=torch.int32) for _ in range(3))
    open_h = torch.zeros(2, device=DEV)
    call("nsid_local_align_strip", p(Sd), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(i32[4]), 2, 4, 9, 0.5, p(i64[1]),
         p(ch), p(ci), p(cj), p(i64[2]), p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(open_h), torch.cuda.current_stream().cuda_stream)
    got = [t.cpu().numpy() for t in rows]
    assert (got[0][:4] == 0).all() and all((got[u][:4] == -1).all() for u in (1, 2, 3))       # min(q_len, max_q_len) rows, empty
    assert all((got[u][4:6] == SENTINEL).all() for u in range(4))                              # nothing past them
    assert open_h.cpu().tolist()[0] == -1 and (ch[:18] == 7).all() and (ci[:18] == 7).all() and (cj[:18] == 7).all()
    want4 = align_chained(S[:4], 0.5, (4,), 40)
    np.testing.assert_array_equal(_bits(got[0][6:]), _bits(want4[0]))
    np.testing.assert_array_equal(got[2][6:], want4[2])
    assert _bits(open_h.cpu().numpy()[1]) == _bits(want4[5][-1]) and not (ch[18:] == 7).all()
    # a run longer than the host said: n_occ = -1 and empty slots
    n32 = _dev(np.asarray([[6, 4], [40, 40]], dtype=np.int32))
    r64 = _dev(np.asarray([0, 6], dtype=np.int64))
    occ = torch.zeros((2, 16, 4), device=DEV, dtype=torch.int32)
    sc = torch.ones((2, 16), device=DEV)
    n_occ = torch.zeros(2, device=DEV, dtype=torch.int32)
    call("nsid_align_occurrences", p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(r64), p(n32[0]), p(n32[1]), 2, 4, 0.0, 16, p(occ),
         p(sc), p(n_occ), torch.cuda.current_stream().cuda_stream)
    w = occurrences_unpacked(want4[0], want4[1], want4[2], want4[3], 40, 0.0, 16)
    assert n_occ.cpu().tolist() == [-1, w[2]] and (occ[0] == -1).all() and (sc[0] == 0).all()
    np.testing.assert_array_equal(occ[1].cpu().numpy(), w[0])


def test_the_profile_books_the_kernels_the_library_took():
    from neuralsampleid_amd import ops
    S = _dev(dyadic(np.random.default_rng(2), 4, 1030).reshape(-1))
    carry, carry_off = ops.align_carry([1030], DEV)
    before = ops.PROFILE
    ops.PROFILE = ops.KernelProfile()
    try:
        r = ops.local_align_strip(S, [0], [1030], [4], [1030], 0.5, [0], [1], carry, carry_off)
        ops.local_align_strip(S, [0], [1030], [4], [9], 0.5, [0], [1], carry, carry_off)
        ops.align_occurrences(*r[:4], [0], [4], [0])
        names = [rec[0] for rec in ops.PROFILE.records]
    finally:
        ops.PROFILE = before
    torch.cuda.synchronize()
    assert names == ["local_align_strip_kernel<1024>", "local_align_strip_kernel<256>", "align_occurrences_kernel"]


# ------------------------------------------------------------------------------------------------ align_occurrences
def _assert_occurrences(ops, runs, firsts, min_score, top):
    """runs: per run (row_h, row_j, row_i0, row_j0) on the host; all of them in one launch against the oracle"""
    n_rows = [len(r[0]) for r in runs]
    row_off = np.cumsum(n_rows) - np.asarray(n_rows)
    dt = (np.float32, np.int32, np.int32, np.int32)
    flat = [_dev(np.concatenate([np.asarray(r[u], dtype=dt[u]) for r in runs] + [np.zeros(1, dt[u])])) for u in range(4)]
    before = ops.launch_counters()["align_occurrences"]
    occ, sc, n_occ = (t.cpu().numpy() for t in ops.align_occurrences(*flat, row_off, n_rows, firsts, min_score, top))
    assert ops.launch_counters()["align_occurrences"] == before + 1
    assert occ.shape == (len(runs), top, 4) and sc.shape == (len(runs), top)
    over = 0
    for p, r in enumerate(runs):
        want = occurrences_unpacked(*r, firsts[p], min_score, top)
        assert n_occ[p] == want[2], p
        np.testing.assert_array_equal(occ[p], want[0], err_msg=f"run {p}")            # unused slots too
        np.testing.assert_array_equal(_bits(sc[p]), _bits(want[1]), err_msg=f"run {p}")
        over += want[2] > top
    return over, n_occ


@pytest.mark.parametrize("top", [1, 16, 64])
def test_occurrences_of_the_strip_rows(strip_cases, top):
    from neuralsampleid_amd import ops
    firsts = [ROW_BASES[p % 4] for p in range(len(STRIP_PAIRS))]
    runs = [(w[0], w[1], np.where(w[2] >= 0, w[2] + f, -1), w[3]) for (_, _, _, w), f in zip(strip_cases, firsts)]
    over, n_occ = _assert_occurrences(ops, runs, firsts, 0.0, top)
    assert over >= (2 if top < 64 else 0) and n_occ.max() > 16
    _assert_occurrences(ops, runs, firsts, 0.75, top)                  # min_score drops whole groups
    assert _assert_occurrences(ops, runs, firsts, 100.0, top)[1].max() == 0


def _hand_made_run(n=20000, first=5000, groups=300, seed=3):
    """a run of n rows: groups of rows with one origin each, spread over up to the whole window [i0, i0 + 8190] of their origin; scores on
    a grid of 0.25, so ties abound; origins that share i0 or j0; one group whose best row is the last of its window"""
    rng = np.random.default_rng(seed)
    row_h = np.zeros(n, np.float32)
    row_j = np.full(n, -1, np.int32)
    row_i0 = np.full(n, -1, np.int32)
    row_j0 = np.full(n, -1, np.int32)
    free = np.ones(n, dtype=bool)

    def put(i0, j0, rows, scores):
        for r, s in zip(rows, scores):
            if r < n and free[r]:
                free[r] = False
                row_h[r], row_j[r], row_i0[r], row_j0[r] = s, j0 + (r - i0) // 2, first + i0, j0
    put(100, 7, [100, 4000, 100 + 8190], [1.0, 1.0, 1.25])             # the best row at the end of the window
    put(100, 8, [101, 102, 103], [1.25, 1.25, 1.0])                    # the same i0, another j0; a tie inside the group (the smaller i)
    put(101, 7, [104, 105], [1.25, 0.5])                               # the same j0, another i0; ties in score between groups
    put(n - 1, 0, [n - 1], [2.0])                                      # the last row alone
    put(0, 0, [0], [2.0])                                              # and the first
    for _ in range(groups):
        i0 = int(rng.integers(0, n))
        j0 = int(rng.integers(0, 4096))
        span = int(rng.choice([3, 40, 900, 8190]))
        k = int(rng.integers(1, 12))
        rows = np.unique(np.minimum(i0 + rng.integers(0, span + 1, size=k), n - 1))
        put(i0, j0, [i0] + rows.tolist(), (rng.integers(1, 13, size=rows.size + 1) * 0.25).astype(np.float32))
    return row_h, row_j, row_i0, row_j0


@pytest.mark.parametrize("top", [1, 16, 64])
def test_occurrences_of_a_long_run(top):
    from neuralsampleid_amd import ops
    long_run = _hand_made_run()
    few = tuple(a[:200].copy() for a in _hand_made_run(200, 5000, 2, seed=4))     # fewer occurrences than top = 16: unused slots
    none = (np.zeros(50, np.float32),) + tuple(np.full(50, -1, np.int32) for _ in range(3))
    empty = (np.zeros(0, np.float32),) + tuple(np.zeros(0, np.int32) for _ in range(3))
    runs, firsts = [long_run, few, none, empty, long_run], [5000, 5000, 0, 0, 5000]
    over, n_occ = _assert_occurrences(ops, runs, firsts, 0.0, top)
    assert over >= 2 and n_occ[0] > 64 and 0 < n_occ[1] < 16 and n_occ[2] == 0 and n_occ[3] == 0
    _, n_kept = _assert_occurrences(ops, runs, firsts, 1.75, top)
    assert 0 < n_kept[0] < n_occ[0]
    # the groups are what the window is for: many rows of one origin far from each other, and rows of other groups in between
    h, j, i0, j0 = long_run
    far = [(i0 == g).nonzero()[0] for g in np.unique(i0[i0 >= 0])]
    assert max(int(r.max() - r.min()) for r in far) == 8190


# ------------------------------------------------------------------------------------------------ SampleIndex.scanner / scan
def _as_tuples(occs):
    return [(o.song, o.q_rows, o.r_rows, _bits(np.float32(o.score)).item()) for o in occs]


ALIGN_LQ = 300
ALIGN_PLANTS = [(15, 20, 12, 1.0), (100, 60, 16, 0.75), (190, 10, 10, 1.5), (270, 20, 12, 1.0)]


@pytest.fixture(scope="module")
def three_songs():
    from neuralsampleid_amd.identify import SampleIndex
    q, ref = case(1, ALIGN_LQ, 90, 128, ALIGN_PLANTS, PLANT_NOISE)
    rng = np.random.default_rng(128)
    idx = SampleIndex(None, device=DEV)
    songs = {"other 0": smooth_rows(rng, 70, 128), "planted": ref, "other 1": smooth_rows(rng, 33, 128)}
    for name, rows in songs.items():
        idx.add_rows(name, _dev(rows))
    return idx, _dev(q), list(songs)


@pytest.mark.parametrize("window_rows", [16, 33, 300])
def test_scanner_with_named_songs_is_align_in_strips(three_songs, window_rows):
    from neuralsampleid_amd import ops
    idx, q, names = three_songs
    per_song, rows = idx.align(q, names, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, return_rows=True, row_hop_s=0.5,
                               row_len_s=1.0)
    assert len(per_song[1]) == 4
    want = sorted(((idx.code(n), o) for n, occs in zip(names, per_song) for o in occs),
                  key=lambda t: (-t[1].score, t[0], t[1].q_rows[0], t[1].r_rows[0]))
    before = ops.launch_counters()
    sc = idx.scanner(threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, window_rows=window_rows, songs=names, row_hop_s=0.5,
                     row_len_s=1.0)
    sc.push(q)
    got = sc.finish()
    after = ops.launch_counters()
    assert got == [o for _, o in want]                                 # the same tuples, times and score bits
    W = sc.window_rows
    assert W == min(window_rows, ops.VOTE_MAX_CAND // 20)
    windows = -(-ALIGN_LQ // W)
    assert sc.stats == {"windows": windows, "strips": 3 * windows, "runs": 3, "rows": ALIGN_LQ, "closed_at_cap": 0}
    assert after["flat_l2_topk"] == before["flat_l2_topk"] and after["song_vote"] == before["song_vote"]        # nothing is voted
    assert after["pair_sim"] == before["pair_sim"] + windows and after["local_align_strip"] == before["local_align_strip"] + windows
    assert after["align_occurrences"] == before["align_occurrences"] + 1
    assert [t["active"] for t in sc.trace] == [[idx.code(n) for n in names]] * windows and all(t["vote_codes"] == [] for t in sc.trace)
    chunk = rows["chunks"][0]
    row_h, row_j, row_org, row_off = chunk[5].cpu().numpy(), chunk[6].cpu().numpy(), chunk[7].cpu().numpy(), chunk[8]
    assert [r["song"] for r in sc.runs] == names
    for p, r in enumerate(sc.runs):
        a, b = int(row_off[p]), int(row_off[p]) + ALIGN_LQ
        assert r["first_row"] == 0 and r["n_rows"] == ALIGN_LQ
        np.testing.assert_array_equal(_bits(r["row_h"].cpu().numpy()), _bits(row_h[a:b]))
        np.testing.assert_array_equal(r["row_j"].cpu().numpy(), row_j[a:b])
        i0, j0 = r["row_i0"].cpu().numpy(), r["row_j0"].cpu().numpy()
        np.testing.assert_array_equal(np.where(i0 >= 0, i0 << 16 | j0, -1), row_org[a:b])
    assert idx.scan(fp=q, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, window_rows=window_rows, songs=names, row_hop_s=0.5,
                    row_len_s=1.0) == got


VOTED_SONGS = [40, 90, 55, 70, 64, 48]                              # rows of the six songs
# (recording row, song, song row, rows, rate): across the window boundary at row 64; stretched; inside the last, partial window.
# Each starts on the second row of a window. The vote is identify_pairs' (the reference's sequence score): a candidate's score is the
# mean of q[window start + i] . x[candidate + i], so a song collects a total above the noise of the others only from the candidates of
# a window's first rows (neighbouring rows correlate over 8 rows here); an excerpt that starts deep inside a window is seen by the vote
# of the NEXT window, if it reaches it, and its first rows are then missed. That is the vote's rule, not the scanner's: the scanner
# is held to its own rule by the trace replay and the row results below, whatever the vote says.
VOTED_PLANTS = [(33, 1, 10, 38, 1.0), (161, 3, 5, 14, 1.5), (385, 4, 20, 12, 1.0)]


def _recording(rng, songs, n, plants, d=128):
    q = smooth_rows(rng, n, d)
    for a, s, b, rows, rate in plants:
        for t in range(rows):
            v = songs[s][b + int(round(t * rate))] + PLANT_NOISE * rng.standard_normal(d) / np.sqrt(d)
            q[a + t] = (v / np.linalg.norm(v)).astype(np.float32)
    return q


def _plant_found(occs, names, plant):
    a, s, b, rows, rate = plant
    want = (a, a + rows - 1, b, b + int(round((rows - 1) * rate)))
    hits = [o for o in occs if o.song == names[s] and all(abs(g - w) <= 1 for g, w in zip(o.q_rows + o.r_rows, want))]
    return len(hits) == 1


@pytest.fixture(scope="module")
def six_songs():
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.default_rng(2024)
    songs = [smooth_rows(rng, n, 128) for n in VOTED_SONGS]
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_dev(smooth_rows(rng, 40, 128)))
    for s, rows in enumerate(songs):
        idx.add_rows(f"song {s}", _dev(rows))
    return idx, songs, rng


def _assert_trace_obeys_the_rule(sc, n_songs, max_active):
    votes = [t["vote_codes"] for t in sc.trace]
    opens = [dict(zip(t["active"], t["open_h"])) for t in sc.trace]
    active, closed, runs = replay_active(votes, opens, n_songs, max_active)
    assert [t["active"] for t in sc.trace] == active
    assert sc.stats["closed_at_cap"] == closed and sc.stats["runs"] == len(runs)
    assert sc.stats["strips"] == sum(len(a) for a in active) and sc.stats["windows"] == len(sc.trace)
    starts = [t["start"] for t in sc.trace]
    ends = [t["start"] + t["rows"] for t in sc.trace]
    assert sorted((r["code"], r["first_row"], r["first_row"] + r["n_rows"]) for r in sc.runs) == \
        sorted((c, starts[t0], ends[t1]) for c, t0, t1 in runs)
    return runs


def test_voted_scan(six_songs):
    from neuralsampleid_amd import ops
    idx, songs, _ = six_songs
    names = idx.names
    q = _recording(np.random.default_rng(7), songs, 400, VOTED_PLANTS)
    qd = _dev(q)
    kw = dict(threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, window_rows=32, k_probe=5, n_songs=2, row_hop_s=0.5, row_len_s=1.0)
    sc = idx.scanner(**kw)
    before = ops.launch_counters()
    sc.push(qd)
    occs = sc.finish()
    after = ops.launch_counters()
    assert len(sc.trace) == 13 and [t["rows"] for t in sc.trace] == [32] * 12 + [16] and sc.stats["rows"] == 400
    assert [t["start"] for t in sc.trace] == list(range(0, 400, 32))
    assert after["song_vote"] == before["song_vote"] + 13 and after["local_align_strip"] == before["local_align_strip"] + 13
    assert after["align_occurrences"] == before["align_occurrences"] + 1
    assert all(len(t["vote_codes"]) <= 2 and len(t["vote_codes"]) == len(t["vote_totals"]) for t in sc.trace)
    runs = _assert_trace_obeys_the_rule(sc, 2, 64)
    assert any(t1 > t0 for _, t0, t1 in runs)                          # a run of more than one window
    # every run's rows are the rule on pair_sim's S of the run's rows, whatever the windows
    for r in sc.runs:
        lo, n, Lr = r["first_row"], r["n_rows"], VOTED_SONGS[r["code"]]
        S, _, _ = ops.pair_sim(qd, idx.fingerprints, [lo], [n], [idx._song_rows[r["code"]][0]], [Lr])
        want = align_chained(S.cpu().numpy().reshape(n, Lr), PLANT_THETA, (n,), lo)
        np.testing.assert_array_equal(_bits(r["row_h"].cpu().numpy()), _bits(want[0]))
        for u, key in ((1, "row_j"), (2, "row_i0"), (3, "row_j0")):
            np.testing.assert_array_equal(r[key].cpu().numpy(), want[u])
    for plant in VOTED_PLANTS:
        assert _plant_found(occs, names, plant), (plant, occs)
    first = [o for o in occs if o.song == names[1]][0]
    assert first.q_rows[0] < 64 <= first.q_rows[1]                     # one occurrence across the window boundary, found once
    assert [(-o.score) for o in occs] == sorted(-o.score for o in occs)
    assert first.q_time == (first.q_rows[0] * 0.5, first.q_rows[1] * 0.5 + 1.0)
    # the cuts of the pushes change nothing
    sc2 = idx.scanner(**kw)
    lo = 0
    for n in (1, 7, 100, 0, 292):
        sc2.push(qd[lo:lo + n])
        lo += n
    assert sc2.finish() == occs and sc2.trace == sc.trace and sc2.stats == sc.stats
    assert idx.scan(fp=qd, **kw) == occs
    # exclude goes to the vote
    sc3 = idx.scanner(exclude=names[1], **kw)
    sc3.push(qd)
    assert all(o.song != names[1] for o in sc3.finish()) and all(1 not in t["vote_codes"] for t in sc3.trace)


def test_scan_of_a_recording_past_the_row_limit(six_songs):
    """locate refuses 4200 rows; scan finds a plant that lies across row 4096 and one wholly behind it"""
    idx, songs, _ = six_songs
    plants = [(4090, 1, 10, 41, 1.0), (4150, 3, 5, 14, 1.5)]
    kw = dict(threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, n_songs=len(VOTED_SONGS))     # every song that votes is aligned
    qd = _dev(_recording(np.random.default_rng(11), songs, 4200, plants))
    with pytest.raises(ValueError, match="4096"):
        idx.locate(fp=qd, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE)
    occs = idx.scan(fp=qd, **kw)
    for plant in plants:
        assert _plant_found(occs, idx.names, plant), (plant, occs)
    across = [o for o in occs if o.song == idx.names[1]][0]
    behind = [o for o in occs if o.song == idx.names[3]][0]
    assert across.q_rows[0] < 4096 < across.q_rows[1] and behind.q_rows[0] > 4096


def test_max_active_closes_the_song_past_the_cap():
    """two songs that hold the same material are open at the same time; with max_active = 1 one of them is closed and counted"""
    from neuralsampleid_amd.identify import SampleIndex
    rng = np.random.default_rng(99)
    songs = [smooth_rows(rng, 60, 128), smooth_rows(rng, 80, 128), smooth_rows(rng, 50, 128)]
    twin = songs[1][10:50] + 0.02 * rng.standard_normal((40, 128)).astype(np.float32)
    songs.append((twin / np.linalg.norm(twin, axis=1, keepdims=True)).astype(np.float32))
    idx = SampleIndex(None, device=DEV)
    for s, rows in enumerate(songs):
        idx.add_rows(f"song {s}", _dev(rows))
    qd = _dev(_recording(np.random.default_rng(5), songs, 160, [(33, 1, 12, 30, 1.0)]))
    kw = dict(threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, window_rows=32, k_probe=5, n_songs=2)
    wide = idx.scanner(**kw)
    wide.push(qd)
    both = wide.finish()
    assert {o.song for o in both} >= {"song 1", "song 3"}
    assert any({1, 3} <= {c for c, h in zip(t["active"], t["open_h"]) if h > 0} for t in wide.trace)      # open at the same time
    assert wide.stats["closed_at_cap"] == 0
    _assert_trace_obeys_the_rule(wide, 2, 64)
    one = idx.scanner(max_active=1, **kw)
    one.push(qd)
    found = one.finish()
    assert all(len(t["active"]) <= 1 for t in one.trace)
    assert one.stats["closed_at_cap"] >= 1
    _assert_trace_obeys_the_rule(one, 2, 1)
    assert len({o.song for o in found} & {"song 1", "song 3"}) >= 1


def test_every_refusal(six_songs):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    idx, songs, _ = six_songs
    q = _dev(smooth_rows(np.random.default_rng(1), 40, 128))
    before = ops.launch_counters()

    def refused(exc, fn, *a, **kw):
        with pytest.raises(exc):
            fn(*a, **kw)
        assert ops.launch_counters() == before

    refused(ValueError, idx.scanner)                                                    # no threshold
    refused(ValueError, idx.scan, fp=q)
    refused(ValueError, idx.scanner, threshold=float("nan"))
    refused(ValueError, idx.scanner, threshold=0.5, min_score=float("nan"))
    refused(ValueError, idx.scanner, threshold=0.5, top=0)
    refused(ValueError, idx.scanner, threshold=0.5, top=65)
    refused(ValueError, idx.scanner, threshold=0.5, songs=["song 0"], exclude="song 1")
    refused(KeyError, idx.scanner, threshold=0.5, songs=["no such song"])
    refused(ValueError, idx.scanner, threshold=0.5, songs=["song 0", "song 0"])
    sc = idx.scanner(threshold=0.5)
    refused(RuntimeError, sc.push, q.cpu())                                             # CPU tensors
    refused(ValueError, sc.push, q[:, :64])                                             # another d than the index holds
    refused(ValueError, sc.push, q.double())
    refused(ValueError, idx.scan, fp=q[:, :64], threshold=0.5)
    # the ops
    S = torch.zeros(72, device=DEV)
    carry, carry_off = ops.align_carry([9], DEV)
    strip = lambda *a, **kw: ops.local_align_strip(*a, **kw)
    refused(ValueError, strip, S, [0], [9], [8], [9], float("nan"), [0], [1], carry, carry_off)
    refused(ValueError, strip, S, [0], [9], [4097], [9], 0.5, [0], [1], carry, carry_off)
    refused(ValueError, strip, S, [0], [9], [8], [4097], 0.5, [0], [1], carry, carry_off)
    refused(ValueError, strip, S, [0], [9], [-1], [9], 0.5, [0], [1], carry, carry_off)
    refused(ValueError, strip, S, [1], [9], [8], [9], 0.5, [0], [1], carry, carry_off)                  # the block leaves S
    refused(ValueError, strip, S, [0], [8], [8], [9], 0.5, [0], [1], carry, carry_off)                  # s_ld < x_len
    refused(ValueError, strip, S, [0], [9], [8], [9], 0.5, [-1], [1], carry, carry_off)                 # row_base
    refused(ValueError, strip, S, [0], [9], [8], [9], 0.5, [2 ** 31 - 8], [1], carry, carry_off)
    refused(ValueError, strip, S, [0], [9], [8], [9], 0.5, [0], [1], carry, [1])                        # the carry leaves its tensors
    refused(ValueError, strip, S, [0, 0], [9, 9], [4, 4], [9, 9], 0.5, [0, 0], [1, 1], ops.align_carry([9, 9], DEV)[0], [0, 9])   # overlap
    refused(ValueError, strip, S, [0], [9], [8], [9], 0.5, [0], [1, 1], carry, carry_off)               # one entry per pair
    refused(RuntimeError, strip, S, [0], [9], [8], [9], 0.5, [0], [1], (carry[0], carry[1].float(), carry[2]), carry_off)
    refused(RuntimeError, strip, S.double(), [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off)
    rows = (torch.zeros(8, device=DEV),) + tuple(torch.zeros(8, device=DEV, dtype=torch.int32) for _ in range(3))
    refused(ValueError, strip, S, [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off, rows=rows, row_off=[1])   # the rows leave their tensors
    refused(ValueError, ops.align_occurrences, *rows, [0], [8], [0], 0.0, 0)
    refused(ValueError, ops.align_occurrences, *rows, [0], [8], [0], 0.0, 65)
    refused(ValueError, ops.align_occurrences, *rows, [0], [8], [0], float("nan"))
    refused(ValueError, ops.align_occurrences, *rows, [0], [9], [0])                                    # the run leaves the rows
    refused(ValueError, ops.align_occurrences, *rows, [0], [8], [-1])
    refused(ValueError, ops.align_occurrences, *rows, [0], [8], [2 ** 31 - 8])
    refused(ValueError, ops.align_occurrences, *rows, [0], [ops.ALIGN_OCC_MAX_ROWS + 1], [0])
    refused(RuntimeError, ops.align_occurrences, rows[0], rows[1].float(), rows[2], rows[3], [0], [8], [0])
    # nothing to do launches nothing
    res = ops.local_align_strip(S, [], [], [], [], 0.5, [], [], carry, [])
    assert res[0].numel() == 0 and res[5].numel() == 0
    assert ops.align_occurrences(*rows, [], [], [])[2].numel() == 0
    assert ops.launch_counters() == before
    # a song past the limit: named, and chosen by a vote
    long_idx = SampleIndex(None, device=DEV)
    long_rows = smooth_rows(np.random.default_rng(3), 4097, 128)
    long_idx.add_rows("long", _dev(long_rows))
    long_idx.add_rows("short", _dev(songs[0]))
    before = ops.launch_counters()
    refused(ValueError, long_idx.scanner, threshold=0.5, songs=["long"])
    sc = long_idx.scanner(threshold=0.5, window_rows=16, k_probe=5)
    with pytest.raises(ValueError, match="4096"):
        sc.push(_dev(long_rows[100:116]))                                               # the vote chooses the long song
    after = ops.launch_counters()
    assert after["pair_sim"] == before["pair_sim"] and after["local_align_strip"] == before["local_align_strip"]
