"""GPU: songs past 4096 rows. local_align_panels against the oracle's chained strips on the whole matrix, bit for bit, whatever the panel
width and the strip cuts; align_occurrences with a span per run; and SampleIndex(long_songs=True): align, scan / scanner and links with
a song that is longer than one workgroup's columns, next to a default index that refuses it as before."""
import numpy as np
import pytest
import torch

from locate_oracle import PLANT_MIN_SCORE, PLANT_NOISE, PLANT_THETA, case, dyadic, plants_matched, smooth_rows
from scan_oracle import align_chained, occurrences_unpacked

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


def _as_tuples(occs):
    return [(o.song, o.q_rows, o.r_rows, _bits(np.float32(o.score)).item(), o.q_time, o.r_time) for o in occs]


# ------------------------------------------------------------------------------------------------ local_align_panels
def _sentinel_rows(n):
    return (torch.full((n,), float(SENTINEL), device=DEV),) + tuple(
        torch.full((n,), SENTINEL, device=DEV, dtype=torch.int32) for _ in range(3))


def _panels(ops, mats, cuts, panel_cols, row_base=0, entry=None):
    """the pairs `mats` (host matrices) through one launch per strip of `cuts` rows (the same cuts for every pair, cut short at a
    pair's end); per pair (rows, carry (h, i0, j0) as (2, Lr), open_h per strip), all on the host"""
    entry = entry or (lambda *a, **kw: ops.local_align_panels(*a, panel_cols=panel_cols, **kw))
    P = len(mats)
    q_tot = np.asarray([m.shape[0] for m in mats], dtype=np.int64)
    x_len = np.asarray([m.shape[1] for m in mats], dtype=np.int64)
    s_size = q_tot * x_len
    s_base = np.cumsum(s_size) - s_size
    S = _dev(np.concatenate([m.reshape(-1) for m in mats] + [np.zeros(1, np.float32)]))
    carry, carry_off = ops.align_carry(x_len, DEV, long_songs=True)
    r_base = np.cumsum(q_tot) - q_tot
    rows = _sentinel_rows(int(q_tot.sum()) + 1)
    done = np.zeros(P, dtype=np.int64)
    started = np.zeros(P, dtype=bool)
    opens = []
    for n in cuts:
        q_len = np.minimum(n, q_tot - done)
        res = entry(S, s_base + done * x_len, x_len, q_len, x_len, 0.5, row_base + done, (~started).astype(np.int64), carry, carry_off,
                    rows=rows, row_off=r_base + done)
        opens.append(res[5].cpu().numpy())
        done += q_len
        started |= q_len > 0
    assert (done == q_tot).all()
    host = [t.cpu().numpy() for t in rows]
    assert all((h[-1] == SENTINEL) for h in host)                        # nothing past the last pair's rows
    ch, ci, cj = (t.cpu().numpy() for t in carry)
    out = []
    for p in range(P):
        a, b, co, Lr = int(r_base[p]), int(r_base[p] + q_tot[p]), int(carry_off[p]), int(x_len[p])
        out.append(([h[a:b] for h in host], tuple(c[co:co + 2 * Lr].reshape(2, Lr) for c in (ch, ci, cj)), [o[p] for o in opens]))
    return out


def _assert_equal(got, want, msg, carry=True):
    rows, cr, opens = got
    np.testing.assert_array_equal(_bits(rows[0]), _bits(want[0]), err_msg=msg)
    for u in (1, 2, 3):
        np.testing.assert_array_equal(rows[u], want[u], err_msg=f"{msg} rows[{u}]")
    if carry:
        np.testing.assert_array_equal(_bits(cr[0]), _bits(want[4][0]), err_msg=msg)
        np.testing.assert_array_equal(cr[1], want[4][1], err_msg=msg)
        np.testing.assert_array_equal(cr[2], want[4][2], err_msg=msg)
    assert [_bits(o).item() for o in opens] == [_bits(o).item() for o in want[5]], msg


# (Lq, Lr, panel_cols): five panels with a partial last one; a last panel of 64, 1 and 2 columns; the narrowest panels; both workgroup
# sizes (panel_cols <= 1024: 256 threads); one panel
DYADIC_CASES = [(150, 300, 64), (150, 128, 64), (150, 129, 64), (150, 130, 64), (40, 9, 2), (150, 1030, 256), (150, 1030, 1024),
                (150, 64, 64)]


@pytest.fixture(scope="module")
def dyadic_cases():
    """per shape (S, the oracle's whole-matrix result from fresh), computed once"""
    rng = np.random.default_rng(4096)
    out = {}
    for Lq, Lr, _ in DYADIC_CASES:
        if (Lq, Lr) not in out:
            S = dyadic(rng, Lq, Lr)
            out[(Lq, Lr)] = (S, align_chained(S, 0.5, (Lq,), 0))
    return out


@pytest.mark.parametrize("Lq,Lr,pc", DYADIC_CASES)
def test_panels_equal_the_rule_on_the_whole_matrix(dyadic_cases, Lq, Lr, pc):
    from neuralsampleid_amd import ops
    S, want = dyadic_cases[(Lq, Lr)]
    before = ops.launch_counters()
    got = _panels(ops, [S], (Lq,), pc)[0]
    after = ops.launch_counters()
    assert after["local_align_panels"] == before["local_align_panels"] + 1 and after["local_align_strip"] == before["local_align_strip"]
    _assert_equal(got, want, f"{Lq} x {Lr} in panels of {pc}")
    if Lr <= pc:                                                       # one panel: the strip kernel's outputs too
        strip = _panels(ops, [S], (Lq,), pc, entry=lambda *a, **kw: ops.local_align_strip(*a, **kw))[0]
        _assert_equal(got, (strip[0][0], strip[0][1], strip[0][2], strip[0][3], strip[1], strip[2]), "the strip kernel")


@pytest.mark.parametrize("Lr", [4097, 8193, 16384])
def test_panels_at_the_production_width(Lr):
    from neuralsampleid_amd import ops
    S = dyadic(np.random.default_rng(Lr), 24, Lr)
    want = align_chained(S, 0.5, (24,), 0)
    _assert_equal(_panels(ops, [S], (24,), 4096)[0], want, f"24 x {Lr}")


def test_panels_chained_over_strips_of_every_small_length(dyadic_cases):
    from neuralsampleid_amd import ops
    S, _ = dyadic_cases[(150, 300)]
    cuts = (0, 1, 2, 8, 1, 138)
    want = align_chained(S, 0.5, cuts, 1000)
    got = _panels(ops, [S], cuts, 64, row_base=1000)[0]
    _assert_equal(got, want, "strips 0, 1, 2, 8, 1, 138 from row 1000")
    whole = _panels(ops, [S], (150,), 64, row_base=1000)[0]              # the single strip: the same rows and the same carry
    _assert_equal((whole[0], whole[1], whole[2]), want[:5] + (want[5][-1:],), "one strip from row 1000")


def test_the_result_does_not_depend_on_panel_cols(dyadic_cases):
    from neuralsampleid_amd import ops
    S, want = dyadic_cases[(150, 300)]
    got = [_panels(ops, [S], (150,), pc)[0] for pc in (2, 64, 4096)]
    for g in got:
        _assert_equal(g, want, "panel_cols 2, 64, 4096")


def test_a_path_across_a_strip_edge_and_a_panel_edge_in_one_step():
    """a planted diagonal through (row 75, column 64), a strip cut at row 75 and panels of 64 columns: the step (74, 63) -> (75, 64)
    leaves a strip and a panel at once, and every later row of the plant still names its first cell"""
    from neuralsampleid_amd import ops
    S = np.zeros((150, 300), dtype=np.float32)
    t = np.arange(-20, 21)
    S[75 + t, 64 + t] = 1.0
    want = align_chained(S, 0.5, (75, 75), 0)
    got = _panels(ops, [S], (75, 75), 64)[0]
    _assert_equal(got, want, "the planted diagonal")
    on = np.arange(55, 96)
    assert (got[0][2][on] == 55).all() and (got[0][3][on] == 44).all() and (got[0][1][on] == on - 11).all()
    assert (got[0][0][on] == 0.5 * (on - 54)).all()
    assert (np.delete(got[0][2], on) == -1).all()


def test_one_launch_with_mixed_pairs():
    """lengths 0 on either side and different x_len per pair: each pair's result is its result in a launch of its own. A pair whose
    device lengths exceed the host maxima (the C entry called directly) reads nothing, writes empty rows, leaves its carry and gets
    open_h = -1; its neighbour is not disturbed"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import call
    rng = np.random.default_rng(12)
    mats = [dyadic(rng, 40, 150), np.zeros((0, 70), np.float32), np.zeros((30, 0), np.float32), dyadic(rng, 33, 70), dyadic(rng, 40, 9)]
    before = ops.launch_counters()["local_align_panels"]
    together = _panels(ops, mats, (25, 15), 64)
    assert ops.launch_counters()["local_align_panels"] == before + 2
    for p, m in enumerate(mats):
        alone = _panels(ops, [m], (25, 15), 64)[0]
        want = align_chained(m, 0.5, (min(25, m.shape[0]), max(0, m.shape[0] - 25)), 0)
        _assert_equal(together[p], want, f"pair {p}", carry=m.shape[0] > 0)
        _assert_equal(alone, want, f"pair {p} alone", carry=m.shape[0] > 0)
    # device lengths past the host maxima: pair 0 says 6 x 9 where the host said at most 4 rows; pair 1 is in order (4 rows)
    S = dyadic(rng, 6, 9)
    want4 = align_chained(S[:4], 0.5, (4,), 40)
    Sd = _dev(S.reshape(-1))
    p = lambda t: t.data_ptr()
    i32 = _dev(np.asarray([[9, 9], [6, 4], [9, 9], [40, 40], [1, 1]], dtype=np.int32))        # s_ld, q_len, x_len, row_base, fresh
    i64 = _dev(np.asarray([[0, 0], [0, 18], [0, 6], [0, 16]], dtype=np.int64))                # s_off, carry_off, row_off, halo_off
    ch = torch.full((36,), 7.0, device=DEV)
    ci, cj = (torch.full((36,), 7, device=DEV, dtype=torch.int32) for _ in range(2))
    hh = torch.full((32,), 7.0, device=DEV)
    hi, hj = (torch.full((32,), 7, device=DEV, dtype=torch.int32) for _ in range(2))
    rows = _sentinel_rows(10)
    open_h = torch.zeros(2, device=DEV)
    call("nsid_local_align_panels", p(Sd), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(i32[4]), 2, 4, 9, 4, 0.5, p(i64[1]),
         p(ch), p(ci), p(cj), p(i64[3]), p(hh), p(hi), p(hj), p(i64[2]), p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(open_h),
         torch.cuda.current_stream().cuda_stream)
    got = [t.cpu().numpy() for t in rows]
    assert (got[0][:4] == 0).all() and all((got[u][:4] == -1).all() for u in (1, 2, 3))       # min(q_len, max_q_len) rows, empty
    assert all((got[u][4:6] == SENTINEL).all() for u in range(4))                              # nothing past them
    assert open_h.cpu().tolist()[0] == -1 and (ch[:18] == 7).all() and (ci[:18] == 7).all() and (cj[:18] == 7).all()
    assert (hh[:16] == 7).all() and (hi[:16] == 7).all()                                       # nor its halo
    np.testing.assert_array_equal(_bits(got[0][6:]), _bits(want4[0]))
    for u in (1, 2, 3):
        np.testing.assert_array_equal(got[u][6:], want4[u])
    assert _bits(open_h.cpu().numpy()[1]) == _bits(want4[5][-1])


def test_the_ops_refuse_on_the_device_and_book_their_kernels():
    from neuralsampleid_amd import ops
    S = torch.zeros(72, device=DEV)
    carry, carry_off = ops.align_carry([9], DEV, long_songs=True)
    before = ops.launch_counters()

    def refused(exc, *a, **kw):
        with pytest.raises(exc):
            ops.local_align_panels(*a, **kw)
        assert ops.launch_counters() == before

    refused(ValueError, S, [0], [9], [8], [9], float("nan"), [0], [1], carry, carry_off)
    refused(ValueError, S, [0], [9], [4097], [9], 0.5, [0], [1], carry, carry_off)
    refused(ValueError, S, [0], [16385], [1], [16385], 0.5, [0], [1], carry, carry_off)
    refused(ValueError, S, [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off, panel_cols=1)
    refused(ValueError, S, [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off, panel_cols=4097)
    refused(ValueError, S, [0], [9], [8], [9], 0.5, [0], [1], carry, [1])                   # the carry leaves its tensors
    rows = (torch.zeros(8, device=DEV),) + tuple(torch.zeros(8, device=DEV, dtype=torch.int32) for _ in range(3))
    with pytest.raises(ValueError):
        ops.align_occurrences(*rows, [0], [8], [0], span=[-1])
    with pytest.raises(ValueError):
        ops.align_occurrences(*rows, [0], [8], [0], span=[1, 2])
    res = ops.local_align_panels(S, [], [], [], [], 0.5, [], [], carry, [])
    assert res[0].numel() == 0 and res[5].numel() == 0
    assert ops.launch_counters() == before
    prof = ops.PROFILE
    ops.PROFILE = ops.KernelProfile()
    try:
        r = ops.local_align_panels(S, [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off, panel_cols=4)
        ops.local_align_panels(S, [0], [9], [8], [9], 0.5, [0], [1], carry, carry_off)
        ops.align_occurrences(*r[:4], [0], [8], [0], span=[16])
        names = [rec[0] for rec in ops.PROFILE.records]
    finally:
        ops.PROFILE = prof
    torch.cuda.synchronize()
    assert names == ["local_align_panels_kernel<256>", "local_align_panels_kernel<1024>", "align_occurrences_kernel"]


# ------------------------------------------------------------------------------------------------ align_occurrences with a span
def _span_run():
    """9000 rows: rows 0 and 8999 share the origin (0, 5), the larger row_h at 8999 (a group as wide as a song of 4501 rows allows, past
    the 8190 rows of the entry without a span); other groups in between, ties included"""
    n = 9000
    h = np.zeros(n, np.float32)
    j = np.full(n, -1, np.int32)
    i0 = np.full(n, -1, np.int32)
    j0 = np.full(n, -1, np.int32)

    def put(r, hv, g, jv):
        h[r], i0[r], j0[r], j[r] = hv, g[0], g[1], jv
    put(0, 3.0, (0, 5), 6)
    put(8999, 4.5, (0, 5), 4400)
    for r in (100, 101, 102):                                          # a tie inside a group: the smallest row wins
        put(r, 2.5, (90, 7), 20 + r)
    put(4000, 4.5, (3990, 1), 30)                                      # a tie between groups: by i0
    put(4001, 4.5, (3990, 0), 31)                                      # ... and then by j0
    put(8998, 1.0, (8998, 3), 3)
    put(8500, 0.25, (8400, 2), 90)                                     # below min_score
    return h, j, i0, j0


def test_occurrences_with_a_span():
    from neuralsampleid_amd import ops
    run = _span_run()
    want = occurrences_unpacked(*run, 0, 0.5, 16)
    assert want[2] == 5 and want[0][0].tolist() == [0, 8999, 5, 4400]                      # that group is one occurrence ending at 8999
    flat = [_dev(a) for a in run]
    before = ops.launch_counters()
    for span in (8999, 9000, 2 ** 20):
        occ, sc, n_occ = (t.cpu().numpy() for t in ops.align_occurrences(*flat, [0], [9000], [0], 0.5, 16, span=[span]))
        assert n_occ[0] == want[2], span
        np.testing.assert_array_equal(occ[0], want[0], err_msg=str(span))
        np.testing.assert_array_equal(_bits(sc[0]), _bits(want[1]), err_msg=str(span))
    after = ops.launch_counters()
    assert after["align_occurrences_span"] == before["align_occurrences_span"] + 3 and after["align_occurrences"] == before["align_occurrences"]
    # span = None is the entry as it was: its window is 8190 rows, so rows 0 and 8999 do not meet
    none = [t.cpu().numpy() for t in ops.align_occurrences(*flat, [0], [9000], [0], 0.5, 16)]
    same = [t.cpu().numpy() for t in ops.align_occurrences(*flat, [0], [9000], [0], 0.5, 16, span=[8190])]
    assert ops.launch_counters()["align_occurrences"] == after["align_occurrences"] + 1
    assert none[2][0] == 6
    for a, b in zip(none, same):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_several_runs_with_different_spans_in_one_launch():
    from neuralsampleid_amd import ops
    run = _span_run()
    flat = [_dev(np.concatenate([a, a, a[:200], a])) for a in run]
    row_off, n_rows, first = [0, 9000, 18000, 18200], [9000, 9000, 200, 9000], [0, 0, 0, 0]
    before = ops.launch_counters()["align_occurrences_span"]
    occ, sc, n_occ = (t.cpu().numpy() for t in ops.align_occurrences(*flat, row_off, n_rows, first, 0.5, 16, span=[8999, 8190, 12, 2 ** 20]))
    assert ops.launch_counters()["align_occurrences_span"] == before + 1
    whole = occurrences_unpacked(*run, 0, 0.5, 16)
    head = occurrences_unpacked(*[a[:200] for a in run], 0, 0.5, 16)
    assert n_occ.tolist() == [whole[2], whole[2] + 1, head[2], whole[2]]
    for p, want in ((0, whole), (2, head), (3, whole)):
        np.testing.assert_array_equal(occ[p], want[0], err_msg=f"run {p}")
        np.testing.assert_array_equal(_bits(sc[p]), _bits(want[1]), err_msg=f"run {p}")
    assert [0, 0, 5, 6] in occ[1].tolist() and [0, 8999, 5, 4400] in occ[1].tolist()       # the narrow window cuts that group in two


# ------------------------------------------------------------------------------------------------ SampleIndex(long_songs=True)
LONG_SHAPE = (120, 8400, 128)
LONG_PLANTS = [(5, 100, 12, 1.5), (30, 4085, 24, 1.0), (70, 4500, 16, 0.75), (100, 8190, 12, 1.0)]      # two cross columns 4096 and 8192


def _index(songs, long_songs, dummy=None):
    from neuralsampleid_amd.identify import SampleIndex
    idx = SampleIndex(None, device=DEV, long_songs=long_songs)
    if dummy is not None:
        idx.add_dummy(_dev(dummy))
    for name, rows in songs.items():
        idx.add_rows(name, _dev(rows))
    return idx


@pytest.mark.parametrize("seed", range(6))
def test_align_against_a_long_song(seed):
    from neuralsampleid_amd import ops
    q, ref = case(seed, *LONG_SHAPE, LONG_PLANTS, PLANT_NOISE)
    other = smooth_rows(np.random.default_rng(seed + 100), 70, 128)
    idx = _index({"other": other, "long": ref}, True)
    qd = _dev(q)
    before = ops.launch_counters()
    per_song, rows = idx.align(qd, ["other", "long"], threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, return_rows=True)
    after = ops.launch_counters()
    assert after["local_align"] == before["local_align"] + 1 and after["local_align_panels"] == before["local_align_panels"] + 1
    assert after["align_occurrences_span"] == before["align_occurrences_span"] + 1 and after["local_align_strip"] == before["local_align_strip"]
    short, long_ = rows["chunks"]
    assert short[0] == [idx.code("other")] and long_[0] == [idx.code("long")] and len(short) == 12 and len(long_) == 13
    S, _, _ = ops.pair_sim(qd, idx.fingerprints, [0], [120], [idx._song_rows[idx.code("long")][0]], [8400], long_songs=True)
    S = S.cpu().numpy().reshape(120, 8400)
    np.testing.assert_array_equal(_bits(long_[1][0].cpu().numpy()), _bits(S.reshape(-1)))  # the S the chunk reports
    want = align_chained(S, PLANT_THETA, (120,), 0)
    np.testing.assert_array_equal(_bits(long_[5].cpu().numpy()), _bits(want[0]))
    for u in (1, 2, 3):
        np.testing.assert_array_equal(long_[5 + u].cpu().numpy(), want[u])
    occ, sc, n_occ = occurrences_unpacked(*want[:4], 0, PLANT_MIN_SCORE, 16)
    got = per_song[1]
    assert [(o.q_rows[0], o.q_rows[1], o.r_rows[0], o.r_rows[1]) for o in got] == [tuple(r) for r in occ[:min(n_occ, 16)].tolist()]
    assert [_bits(np.float32(o.score)).item() for o in got] == _bits(sc[:len(got)]).tolist()
    assert all(o.song == "long" for o in got)
    assert plants_matched(occ, n_occ, LONG_PLANTS), (seed, occ[:n_occ].tolist())
    # a default index on the same rows refuses the song as before, with nothing launched
    plain = _index({"other": other, "long": ref}, False)
    before = ops.launch_counters()
    with pytest.raises(ValueError, match=r"'long' has 8400 rows, past the limit of 4096"):
        plain.align(qd, ["other", "long"], threshold=PLANT_THETA)
    assert ops.launch_counters() == before


@pytest.fixture(scope="module")
def mix():
    """a catalogue of three short songs and one of 4200 rows that plays rows 5 .. 44 of 'b' from its row 4080 on, across row 4096"""
    rng = np.random.default_rng(31)
    songs = {"a": smooth_rows(rng, 60, 128), "b": smooth_rows(rng, 80, 128), "c": smooth_rows(rng, 50, 128),
             "mix": smooth_rows(rng, 4200, 128)}
    for t in range(40):
        v = songs["b"][5 + t] + PLANT_NOISE * rng.standard_normal(128) / np.sqrt(128)
        songs["mix"][4080 + t] = (v / np.linalg.norm(v)).astype(np.float32)
    dummy = smooth_rows(rng, 40, 128)
    return songs, dummy, _index(songs, True, dummy), _index(songs, False, dummy)


def test_scan_against_a_long_song(mix):
    from neuralsampleid_amd import ops
    songs, _, idx, plain = mix
    rng = np.random.default_rng(32)
    q = smooth_rows(rng, 500, 128)
    for t in range(40):                                                # the second row of the window at 192: song rows 4076 .. 4115
        v = songs["mix"][4076 + t] + PLANT_NOISE * rng.standard_normal(128) / np.sqrt(128)
        q[193 + t] = (v / np.linalg.norm(v)).astype(np.float32)
    qd = _dev(q)
    kw = dict(threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, row_hop_s=0.5, row_len_s=1.0)
    per_song = idx.align(qd, ["mix"], **kw)
    assert len(per_song[0]) >= 1
    best = per_song[0][0]
    assert abs(best.q_rows[0] - 193) <= 1 and abs(best.q_rows[1] - 232) <= 1 and abs(best.r_rows[0] - 4076) <= 1 and \
        abs(best.r_rows[1] - 4115) <= 1 and best.r_rows[0] < 4096 < best.r_rows[1]
    before = ops.launch_counters()
    sc = idx.scanner(songs=["mix"], window_rows=64, **kw)
    sc.push(qd)
    got = sc.finish()
    after = ops.launch_counters()
    assert _as_tuples(got) == _as_tuples(per_song[0])                  # the streaming form of align, bit for bit
    assert after["local_align_panels"] == before["local_align_panels"] + 8 and after["local_align_strip"] == before["local_align_strip"]
    assert after["align_occurrences_span"] == before["align_occurrences_span"] + 1
    # the voted scan: the long song is chosen by the vote and aligned, not refused
    voted = idx.scan(fp=qd, window_rows=64, k_probe=5, n_songs=2, **kw)
    assert _as_tuples([o for o in voted if o.song == "mix"][:1]) == _as_tuples([best])
    # a default index: the same vote ends the scan, as before
    sc = plain.scanner(window_rows=64, k_probe=5, n_songs=2, **kw)
    with pytest.raises(ValueError, match="4096"):
        sc.push(qd)
    before = ops.launch_counters()
    with pytest.raises(ValueError, match="4096"):
        plain.scanner(songs=["mix"], **kw)
    assert ops.launch_counters() == before


def test_the_vote_may_choose_a_song_of_4097_rows():
    """the index of test_scan_gpu.py's last case with long_songs=True: the push that raised there is aligned here"""
    from neuralsampleid_amd import ops
    long_rows = smooth_rows(np.random.default_rng(3), 4097, 128)
    short = smooth_rows(np.random.default_rng(2024), 40, 128)
    idx = _index({"long": long_rows, "short": short}, True)
    before = ops.launch_counters()
    sc = idx.scanner(threshold=0.5, window_rows=16, k_probe=5)
    sc.push(_dev(long_rows[100:116]))                                  # the vote chooses the long song
    occs = sc.finish()
    after = ops.launch_counters()
    assert idx.code("long") in sc.trace[0]["active"] and after["local_align_panels"] == before["local_align_panels"] + 1
    assert occs and occs[0].song == "long" and occs[0].q_rows == (0, 15) and occs[0].r_rows == (100, 115)


def test_links_with_a_long_song(mix):
    songs, _, idx, plain = mix
    kw = dict(k_probe=20, n_songs=3, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16)
    res = idx.links(**kw)
    assert res.skipped == [] and list(res.occurrences) == list(songs)
    there = [o for o in res.occurrences["mix"] if o.song == "b"]
    back = [o for o in res.occurrences["b"] if o.song == "mix"]
    assert len(there) == 1 and len(back) == 1                          # both directions
    assert all(abs(g - w) <= 1 for g, w in zip(there[0].q_rows + there[0].r_rows, (4080, 4119, 5, 44)))
    assert there[0].q_rows[0] < 4096 < there[0].q_rows[1]              # across the edge of the query's two strips
    assert all(abs(g - w) <= 1 for g, w in zip(back[0].q_rows + back[0].r_rows, (5, 44, 4080, 4119)))
    for name in ("mix", "b"):
        lo, n, _ = idx._song_rows[idx.code(name)]
        want = idx.locate(fp=idx.fingerprints[lo:lo + n], leave_out=name, **kw)
        assert _as_tuples(res.occurrences[name]) == _as_tuples(want), name
    # the default index: the long song is skipped, neither queried nor a candidate
    res = plain.links(**kw)
    assert res.skipped == ["mix"] and "mix" not in res.occurrences
    assert all(o.song != "mix" for occs in res.occurrences.values() for o in occs)


def test_refusals_of_the_long_index(mix):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    songs, dummy, idx, plain = mix
    q = _dev(smooth_rows(np.random.default_rng(1), 40, 128))
    before = ops.launch_counters()
    # rerank=True with a long column: refused by the limit (this index has no classifier, which is refused first with another word,
    # so the check is made on an index that has one in name only)
    idx.classifier = object()
    try:
        with pytest.raises(ValueError, match=r"'mix' has 4200 rows, past the limit of 4096"):
            idx._align_checks("align", q, ["mix"], None, 16, None, True)
    finally:
        idx.classifier = None
    with pytest.raises(RuntimeError):
        idx.align(q, ["mix"], rerank=True)
    # a song past 16384 rows: refused by name, skipped by links
    big = SampleIndex(None, device=DEV, long_songs=True)
    assert ops.launch_counters() == before
    big.add_rows("short", _dev(songs["a"]))
    big.add_rows("too long", _dev(smooth_rows(np.random.default_rng(5), 16385, 128)))
    before = ops.launch_counters()
    for fn in (lambda: big.align(q, ["too long"], threshold=0.5), lambda: big.locate(fp=q, songs=["too long"], threshold=0.5),
               lambda: big.scanner(threshold=0.5, songs=["too long"])):
        with pytest.raises(ValueError, match=r"'too long' has 16385 rows.*16384"):
            fn()
    with pytest.raises(ValueError, match="16384"):
        big.align(_dev(np.zeros((16385, 128), np.float32)), ["short"], threshold=0.5)
    assert ops.launch_counters() == before
    res = big.links(k_probe=5, n_songs=1, threshold=PLANT_THETA)
    assert res.skipped == ["too long"] and list(res.occurrences) == ["short"] and res.occurrences["short"] == []
