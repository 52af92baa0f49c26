"""GPU: nsid_align_paths against the path oracle, exactly (end_h and path_s as bit patterns, untouched slots as sentinels): many boxes of
tie-heavy matrices in one launch, every box size at which the kernel takes another path, bad boxes among good ones, global rows, and
SampleIndex.paths."""
import numpy as np
import pytest
import torch

from align_path_oracle import box_path, rows_from, spanning_band, spans, trace
from locate_oracle import PLANT_MIN_SCORE, PLANT_NOISE, PLANT_THETA, STEPS, align_oracle, case, dyadic, smooth_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345
GAP = 3                      # sentinel slots in front of every box's path, and behind the last
LIMIT = 4096


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _seq(v):
    return np.asarray(v, dtype=np.int64).reshape(-1)


def _launch(S, s_off, s_ld, n_rows, n_cols, theta, i_base=None, j_base=None):
    """nsid_align_paths itself, as ops.align_paths calls it, on outputs full of sentinels with gaps between the boxes' slots: (path_len,
    path_off, path_i, path_j, path_s, end_h) on the host"""
    from neuralsampleid_amd import _lib, ops
    s_off, s_ld, n_rows, n_cols = _seq(s_off), _seq(s_ld), _seq(n_rows), _seq(n_cols)
    nb = s_off.size
    i_base = np.zeros(nb, np.int64) if i_base is None else _seq(i_base)
    j_base = np.zeros(nb, np.int64) if j_base is None else _seq(j_base)
    ok = (n_rows <= LIMIT) & (n_cols <= LIMIT)
    slots = np.where(ok, np.minimum(n_rows, n_cols), 0)
    path_off = np.cumsum(slots + GAP) - slots
    total = int((slots + GAP).sum()) + GAP
    dsize = np.where(ok, n_rows * ((n_cols + 3) // 4), 0)
    dir_off = np.cumsum(dsize) - dsize
    max_cols = int(n_cols[ok].max()) if ok.any() else 0
    t32 = _dev(np.stack([s_ld, n_rows, n_cols, i_base, j_base]).astype(np.int32))
    t64 = _dev(np.stack([s_off, path_off, dir_off]))
    path_len = torch.full((nb,), SENTINEL, device=DEV, dtype=torch.int32)
    end_h = torch.full((nb,), float(SENTINEL), device=DEV)
    path_i = torch.full((total,), SENTINEL, device=DEV, dtype=torch.int32)
    path_j = torch.full((total,), SENTINEL, device=DEV, dtype=torch.int32)
    path_s = torch.full((total,), float(SENTINEL), device=DEV)
    dirs = torch.zeros((int(dsize.sum()) + 1,), device=DEV, dtype=torch.uint8)
    before = ops.launch_counters()["align_paths"]
    p = lambda t: t.data_ptr()
    _lib.call("nsid_align_paths", p(S), p(t64[0]), p(t32[0]), p(t32[1]), p(t32[2]), p(t32[3]), p(t32[4]), nb, max_cols, float(theta),
              p(t64[1]), p(t64[2]), p(dirs), p(path_len), p(path_i), p(path_j), p(path_s), p(end_h),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ops.launch_counters()["align_paths"] == before + (1 if nb else 0)
    return tuple(t.cpu().numpy() for t in (path_len,)) + (path_off,) + tuple(t.cpu().numpy() for t in (path_i, path_j, path_s, end_h))


def _check(got, want, sentinels=True):
    """want: per box (status, rows, columns, scores, last H): status = the cells of the path, or 0 / -1 / -2 with no cells; last H None:
    not compared"""
    path_len, path_off, path_i, path_j, path_s, end_h = got
    assert path_len.size == len(want) == end_h.size
    covered = np.zeros(path_i.size, dtype=bool)
    for p, (status, pi, pj, ps, h) in enumerate(want):
        assert path_len[p] == status, (p, int(path_len[p]), status)
        if h is not None:
            assert _bits(end_h[p]) == _bits(h), (p, float(end_h[p]), float(h))
        if status > 0:
            a, b = int(path_off[p]), int(path_off[p]) + status
            covered[a:b] = True
            np.testing.assert_array_equal(path_i[a:b], pi, err_msg=f"box {p}")
            np.testing.assert_array_equal(path_j[a:b], pj, err_msg=f"box {p}")
            np.testing.assert_array_equal(_bits(path_s[a:b]), _bits(ps), err_msg=f"box {p}")
    if sentinels:                                                      # nothing else was written
        assert (path_i[~covered] == SENTINEL).all() and (path_j[~covered] == SENTINEL).all()
        assert (path_s[~covered] == np.float32(SENTINEL)).all()


def _flat(mats, pad=lambda p: (p % 3) * 5, front=7):
    """the matrices in one flat S with NaN between them (what lies outside a box's columns is never read: NaN would show)"""
    q_len, x_len = np.array([m.shape[0] for m in mats]), np.array([m.shape[1] for m in mats])
    s_ld = x_len + np.array([pad(p) for p in range(len(mats))])
    size = q_len * s_ld
    s_off = np.cumsum(size) - size + front
    flat = np.full(int(size.sum()) + front, np.nan, dtype=np.float32)
    for m, o, ld in zip(mats, s_off, s_ld):
        for i in range(m.shape[0]):
            flat[o + i * ld:o + i * ld + m.shape[1]] = m[i]
    return flat, s_off, s_ld, q_len, x_len


# ------------------------------------------------------------------------------------------------ many boxes in one launch
MANY_SHAPES = [(1, 1), (2, 3), (33, 65), (47, 40), (130, 19)]


@pytest.mark.parametrize("theta", [0.375, 0.5])
def test_all_occurrences_of_tie_heavy_matrices_in_one_launch(theta):
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(2025)
    mats = [dyadic(rng, *s) for s in MANY_SHAPES]
    mats[0][0, 0] = 1.0                                                # the 1 x 1 matrix is an occurrence
    flat, s_off, s_ld, q_len, x_len = _flat(mats)
    S = _dev(flat)
    occ, sc, n_occ = (t.cpu().numpy() for t in ops.local_align(S, s_off, s_ld, q_len, x_len, theta, min_score=0.0, top=64)[:3])
    box, want = [], []
    steps_seen = set()
    for p, m in enumerate(mats):
        H, frm = rows_from(m, theta)
        for t in range(min(int(n_occ[p]), 64)):
            i0, i1, j0, j1 = occ[p, t].tolist()
            fi, fj = trace(frm, i1, j1)                                # the path in the whole matrix
            assert (fi[0], fj[0]) == (i0, j0) and _bits(H[i1, j1]) == _bits(sc[p, t])
            box.append((s_off[p] + i0 * s_ld[p] + j0, s_ld[p], i1 - i0 + 1, j1 - j0 + 1, i0, j0))
            want.append((fi.size, fi, fj, m[fi, fj], sc[p, t]))
            steps_seen |= set(zip(np.diff(fi).tolist(), np.diff(fj).tolist()))
    box = np.asarray(box, dtype=np.int64)
    assert len(want) >= 20 and max(w[0] for w in want) >= 8 and min(w[0] for w in want) == 1 and steps_seen == set(STEPS)
    got = _launch(S, box[:, 0], box[:, 1], box[:, 2], box[:, 3], theta, box[:, 4], box[:, 5])
    _check(got, want)
    # ops.align_paths: the same call with its own layout, and the same bits a second time
    before = ops.launch_counters()["align_paths"]
    res = ops.align_paths(S, box[:, 0], box[:, 1], box[:, 2], box[:, 3], theta, i_base=box[:, 4], j_base=box[:, 5])
    assert ops.launch_counters()["align_paths"] == before + 1
    assert np.array_equal(res[1], np.cumsum(np.minimum(box[:, 2], box[:, 3])) - np.minimum(box[:, 2], box[:, 3]))
    assert res[2].numel() == int(np.minimum(box[:, 2], box[:, 3]).sum())
    host = tuple(r if isinstance(r, np.ndarray) else r.cpu().numpy() for r in res)
    _check(host, want, sentinels=False)
    again = ops.align_paths(S, box[:, 0], box[:, 1], box[:, 2], box[:, 3], theta, i_base=box[:, 4], j_base=box[:, 5])
    assert torch.equal(again[0], res[0]) and torch.equal(again[5].view(torch.int32), res[5].view(torch.int32))
    zero = ops.align_paths(S, [], [], [], [], theta)                   # no boxes: nothing is launched
    assert ops.launch_counters()["align_paths"] == before + 2 and zero[0].numel() == 0 and zero[2].numel() == 0


# ------------------------------------------------------------------------------------------------ every size where the kernel changes
# A thread owns 4 neighbouring columns (one byte of step codes): 1, 3, 4 and 5 columns; S is read 8 rows at a time: 7, 8, 9 and 17 rows;
# a wave owns 256 columns: 255, 256, 257; up to 1024 columns the launch has 256 threads, above it 1024: 1023, 1024, 1025; the limit:
# 4095 and 4096 on either side. Each box is a whole spanning band matrix (align_path_oracle.spanning_band), so its sides are the test's.
SMALL = [(1, 1), (5, 1), (2, 3), (3, 3), (3, 4), (3, 5), (4, 4), (5, 5), (5, 3), (7, 7), (8, 8), (9, 9), (9, 16), (17, 9), (130, 255),
         (130, 256), (140, 257), (600, 1023), (600, 1024), (1024, 600)]
SIZE_GROUPS = {"to-1024": (SMALL, "<256>"), "1025": ([(600, 1025), (3, 3), (9, 5), (17, 9)], "<1024>"),
               "2049x4096": ([(2049, 4096)], "<1024>"), "4096x2049": ([(4096, 2049), (5, 5)], "<1024>"),
               "4095x4095": ([(4095, 4095)], "<1024>"), "4096x4096": ([(4096, 4096)], "<1024>"),
               "4095x4096": ([(4095, 4096)], "<1024>"), "4096x4095": ([(4096, 4095)], "<1024>")}


@pytest.mark.parametrize("group", list(SIZE_GROUPS))
def test_box_sizes_where_the_kernel_takes_another_path(group):
    from neuralsampleid_amd import _lib
    shapes, threads = SIZE_GROUPS[group]
    rng = np.random.default_rng(len(group) * 1000 + shapes[0][1])
    theta = 0.375
    mats = [spanning_band(rng, r, c) if spans(r, c) else np.ones((r, c), np.float32) for r, c in shapes]
    flat, s_off, s_ld, q_len, x_len = _flat(mats, pad=lambda p: p % 2)
    i_base, j_base = 1000 * np.arange(len(mats)), 7 * np.arange(len(mats)) + 1
    want = []
    for m, ib, jb in zip(mats, i_base, j_base):
        pi, pj, h = box_path(m, theta, 0, m.shape[0] - 1, 0, m.shape[1] - 1)
        if spans(*m.shape):
            assert pi is not None and pi.size >= min(m.shape) // 2      # one path from corner to corner
            want.append((pi.size, pi + ib, pj + jb, m[pi, pj], h))
        else:
            assert pi is None and h > 0                                 # a column of passing cells: the last one starts its own path
            want.append((-1, None, None, None, h))
    got = _launch(_dev(flat), s_off, s_ld, q_len, x_len, theta, i_base, j_base)
    took = _lib.lib.nsid_debug_last_kernel().decode()
    assert took == "align_paths_kernel" + threads                      # the workgroup goes by the widest box of the launch
    _check(got, want)


# ------------------------------------------------------------------------------------------------ bad boxes among good ones
def test_bad_boxes_among_good_ones_in_one_launch():
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(31)
    theta = 0.5
    m = dyadic(rng, 150, 65)
    ld = 65
    occ, sc, n_occ = align_oracle(m, theta, 0.0, 64)[:3]
    S = _dev(m.reshape(-1))
    box, want = [], []

    def good(t):
        i0, i1, j0, j1 = occ[t].tolist()
        pi, pj, h = box_path(m, theta, i0, i1, j0, j1)
        assert pi is not None and _bits(h) == _bits(sc[t])
        box.append((i0 * ld + j0, ld, i1 - i0 + 1, j1 - j0 + 1, i0, j0))
        want.append((pi.size, pi, pj, m[pi, pj], h))

    n = min(int(n_occ), 64)
    assert n >= 9
    # an occurrence's box moved up by one row that the oracle refuses too
    shifted = next(t for t in range(n) if occ[t, 0] >= 1 and occ[t, 1] > occ[t, 0] and
                   box_path(m, theta, occ[t, 0] - 1, occ[t, 1] - 1, occ[t, 2], occ[t, 3])[0] is None)
    i0, i1, j0, j1 = occ[shifted].tolist()
    bad = {0: ((1 << 40, 3, LIMIT + 1, 3, 0, 0), (-2, None, None, None, np.float32(0))),                 # far outside S: never read
           3: ((0, 5, 0, 5, 0, 0), (0, None, None, None, np.float32(0))),
           5: (((i0 - 1) * ld + j0, ld, i1 - i0 + 1, j1 - j0 + 1, i0 - 1, j0),
               (-1, None, None, None, box_path(m, theta, i0 - 1, i1 - 1, j0, j1)[2])),
           8: ((m.size + 5, LIMIT + 1, 2, LIMIT + 1, 0, 0), (-2, None, None, None, np.float32(0))),
           n: ((0, 0, 6, 0, 0, 0), (0, None, None, None, np.float32(0)))}
    for t in range(n + 1):
        if t in bad:
            box.append(bad[t][0])
            want.append(bad[t][1])
        if t < n:
            good(t)
    box = np.asarray(box, dtype=np.int64)
    assert len(want) == n + 5 and want[-1][0] == 0 and want[0][0] == -2
    got = _launch(S, box[:, 0], box[:, 1], box[:, 2], box[:, 3], theta, box[:, 4], box[:, 5])
    _check(got, want)
    res = ops.align_paths(S, box[:, 0], box[:, 1], box[:, 2], box[:, 3], theta, i_base=box[:, 4], j_base=box[:, 5])
    _check(tuple(r if isinstance(r, np.ndarray) else r.cpu().numpy() for r in res), want, sentinels=False)
    # what ops refuses itself: a box that leaves S, a negative side, a NaN theta, a base past the int32 rows
    before = ops.launch_counters()["align_paths"]
    for kw, exc in ((dict(s_off=[m.size - 10]), ValueError), (dict(n_rows=[-1]), ValueError), (dict(theta=float("nan")), ValueError),
                    (dict(i_base=[2 ** 31 - 3]), ValueError), (dict(s_ld=[2]), ValueError), (dict(n_cols=[3, 3]), ValueError)):
        a = dict(s_off=[0], s_ld=[ld], n_rows=[3], n_cols=[3], theta=theta, i_base=None)
        a.update(kw)
        with pytest.raises(exc):
            ops.align_paths(S, a["s_off"], a["s_ld"], a["n_rows"], a["n_cols"], a["theta"], i_base=a["i_base"])
    assert ops.launch_counters()["align_paths"] == before


# ------------------------------------------------------------------------------------------------ global coordinates
def test_occurrences_of_chained_strips_give_paths_in_global_rows():
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(77)
    Lq, Lr, base, theta = 150, 65, 2 ** 30, 0.5
    m = dyadic(rng, Lq, Lr)
    S = _dev(m.reshape(-1))
    carry, carry_off = ops.align_carry([Lr], DEV)
    rows = (torch.empty((Lq,), device=DEV),) + tuple(torch.empty((Lq,), device=DEV, dtype=torch.int32) for _ in range(3))
    done = 0
    for n in (64, 64, 22):
        ops.local_align_strip(S, [done * Lr], [Lr], [n], [Lr], theta, [base + done], [1 if done == 0 else 0], carry, carry_off,
                              rows=rows, row_off=[done])
        done += n
    occ, sc, n_occ = (t.cpu().numpy() for t in ops.align_occurrences(*rows, [0], [Lq], [base], 0.0, 64))
    k = min(int(n_occ[0]), 64)
    assert k >= 10
    o = occ[0, :k].astype(np.int64)
    assert o[:, 0].min() >= base
    res = ops.align_paths(S, (o[:, 0] - base) * Lr + o[:, 2], [Lr] * k, o[:, 1] - o[:, 0] + 1, o[:, 3] - o[:, 2] + 1, theta,
                          i_base=o[:, 0], j_base=o[:, 2])
    H, frm = rows_from(m, theta)
    want = []
    for (i0, i1, j0, j1), s in zip(o.tolist(), sc[0, :k]):
        fi, fj = trace(frm, i1 - base, j1)
        assert (fi[0] + base, fj[0]) == (i0, j0)
        want.append((fi.size, fi.astype(np.int64) + base, fj, m[fi, fj], s))
    _check(tuple(r if isinstance(r, np.ndarray) else r.cpu().numpy() for r in res), want, sentinels=False)
    assert res[2].max().item() > base


# ------------------------------------------------------------------------------------------------ SampleIndex.paths
LQ = 300
LOCATE_PLANTS = [(15, 20, 12, 1.0), (100, 60, 16, 0.75), (190, 10, 10, 1.5), (270, 20, 12, 1.0)]
HOP_S, LEN_S = 0.5, 1.0


@pytest.fixture(scope="module")
def planted():
    from neuralsampleid_amd.identify import SampleIndex
    q, ref = case(1, LQ, 90, 128, LOCATE_PLANTS, PLANT_NOISE)
    rng = np.random.default_rng(128)
    idx = SampleIndex(None, device=DEV)
    songs = {"other 0": smooth_rows(rng, 70, 128), "planted": ref, "other 1": smooth_rows(rng, 33, 128)}
    for name, rows in songs.items():
        idx.add_rows(name, _dev(rows))
    qd = _dev(q)
    per_song, rows = idx.align(qd, list(songs), threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, top=16, return_rows=True)
    chunk = rows["chunks"][0]
    S = chunk[1].cpu().numpy()
    o, ld = int(chunk[2][1]), int(chunk[3][1])
    mat = S[o + np.arange(LQ)[:, None] * ld + np.arange(90)[None, :]]            # the scores align walked for "planted"
    return idx, qd, list(songs), per_song, mat


def _same(a, b):
    assert a.occurrence == b.occurrence and a.steps == b.steps and a.passing == b.passing
    assert (a.slope, a.intercept, a.rms_rows) == (b.slope, b.intercept, b.rms_rows)
    for u, v in ((a.q_rows, b.q_rows), (a.r_rows, b.r_rows), (a.scores.view(np.int32), b.scores.view(np.int32))):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    for u, v in ((a.q_time, b.q_time), (a.r_time, b.r_time)):
        assert (u is None and v is None) or np.array_equal(u, v)


def test_paths_of_the_planted_case_equal_the_oracle(planted):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import alignment_path
    idx, q, names, per_song, mat = planted
    occs = per_song[1]
    assert len(occs) == 4 and per_song[0] == [] and per_song[2] == []
    before = ops.launch_counters()
    paths = idx.paths(q, occs, PLANT_THETA, row_hop_s=HOP_S, row_len_s=LEN_S)
    after = ops.launch_counters()
    assert after["align_paths"] == before["align_paths"] + 1 and after["pair_sim"] == before["pair_sim"] + 1      # one chunk
    assert len(paths) == 4
    for p, o in zip(paths, occs):
        pi, pj, h = box_path(mat, PLANT_THETA, o.q_rows[0], o.q_rows[1], o.r_rows[0], o.r_rows[1])
        assert pi is not None and _bits(h) == _bits(np.float32(o.score))
        assert p.occurrence is o
        _same(p, alignment_path(o, pi, pj, mat[pi, pj], PLANT_THETA, (HOP_S, LEN_S)))
        assert (p.q_rows[0], p.q_rows[-1]) == o.q_rows and (p.r_rows[0], p.r_rows[-1]) == o.r_rows
        np.testing.assert_array_equal(p.q_time, p.q_rows * HOP_S)
        assert float(p.song_time(p.q_time[0])) == p.r_time[0]
    for a, b, n, rate in LOCATE_PLANTS:                                # a planted query row maps to within one row of its song row
        hit = [p for p in paths if abs(p.q_rows[0] - a) <= 1 and abs(p.r_rows[0] - b) <= 1]
        assert len(hit) == 1
        p = hit[0]
        inside = [t for t in range(n) if p.q_rows[0] <= a + t <= p.q_rows[-1]]
        assert len(inside) >= n - 2
        for t in inside:
            assert abs(float(p.song_row(a + t)) - (b + int(round(t * rate)))) <= 1, (a, t, float(p.song_row(a + t)))
    # any selection in any order, without the timing; none at all launches nothing
    some = idx.paths(q, [occs[2], occs[0]], PLANT_THETA)
    for got, ref in zip(some, (paths[2], paths[0])):
        assert got.q_time is None and got.r_time is None
        _same(got._replace(q_time=ref.q_time, r_time=ref.r_time), ref)
    before = ops.launch_counters()
    assert idx.paths(q, [], PLANT_THETA) == []
    assert ops.launch_counters() == before


def test_a_budget_that_forces_several_chunks_gives_the_same_paths(planted):
    from neuralsampleid_amd import ops
    idx, q, names, per_song, mat = planted
    occs = per_song[1]
    one = idx.paths(q, occs, PLANT_THETA)
    before = ops.launch_counters()["align_paths"]
    cells = [(o.q_rows[1] - o.q_rows[0] + 1) * (o.r_rows[1] - o.r_rows[0] + 1) for o in occs]
    many = idx.paths(q, occs, PLANT_THETA, s_budget_bytes=4 * min(cells))          # no two boxes fit together
    assert ops.launch_counters()["align_paths"] == before + 4
    tiny = idx.paths(q, occs, PLANT_THETA, s_budget_bytes=1)                        # one box is always allowed
    for got in (many, tiny):
        assert len(got) == 4
        for a, b in zip(got, one):
            _same(a, b)


def test_paths_of_scan_occurrences_equal_those_of_align(planted):
    idx, q, names, per_song, mat = planted
    key = lambda o: (o.song, o.q_rows, o.r_rows, _bits(np.float32(o.score)).item())
    by_align = {key(o): o for occs in per_song for o in occs}
    scanned = idx.scan(fp=q, threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE, window_rows=33, songs=names)
    assert len(scanned) == 4 and sorted(map(key, scanned)) == sorted(by_align)
    for a, b in zip(idx.paths(q, scanned, PLANT_THETA), idx.paths(q, [by_align[key(o)] for o in scanned], PLANT_THETA)):
        _same(a._replace(occurrence=b.occurrence), b)


@pytest.fixture(scope="module")
def long_song():
    from neuralsampleid_amd.identify import SampleIndex
    q, ref = case(3, 60, 5000, 64, [(10, 4400, 24, 1.0), (40, 100, 12, 1.5)], PLANT_NOISE)
    idx = SampleIndex(None, device=DEV, long_songs=True)
    idx.add_rows("short", _dev(smooth_rows(np.random.default_rng(1), 50, 64)))
    idx.add_rows("long", _dev(ref))
    return idx, _dev(q), _dev(ref)


def test_paths_in_a_song_past_4096_rows(long_song):
    from neuralsampleid_amd import ops
    idx, q, ref = long_song
    occs = idx.align(q, ["long"], threshold=PLANT_THETA, min_score=PLANT_MIN_SCORE)[0]
    assert len(occs) >= 2 and any(o.r_rows[0] > 4096 for o in occs) and any(o.r_rows[1] < 4096 for o in occs)
    S, _, _ = ops.pair_sim(q, ref, [0], [60], [0], [5000], long_songs=True)      # an element's bits depend on its two rows alone
    mat = S.cpu().numpy().reshape(60, 5000)
    paths = idx.paths(q, occs, PLANT_THETA)
    for p, o in zip(paths, occs):
        pi, pj, h = box_path(mat, PLANT_THETA, o.q_rows[0], o.q_rows[1], o.r_rows[0], o.r_rows[1])
        assert pi is not None and _bits(h) == _bits(np.float32(o.score))
        assert np.array_equal(p.q_rows, pi) and np.array_equal(p.r_rows, pj) and np.array_equal(_bits(p.scores), _bits(mat[pi, pj]))
    far = next(p for p in paths if p.r_rows[0] > 4096)
    assert abs(far.slope - 1.0) <= 0.1 and abs(float(far.song_row(20)) - 4410) <= 1


def test_every_refusal_of_paths(planted, long_song):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import Occurrence
    idx, q, names, per_song, mat = planted
    occs = per_song[1]
    o = occs[0]
    before = ops.launch_counters()
    with pytest.raises(RuntimeError, match="no CPU path"):
        idx.paths(q.cpu(), occs, PLANT_THETA)
    with pytest.raises(ValueError, match="threshold"):
        idx.paths(q, occs)
    with pytest.raises(ValueError, match="NaN"):
        idx.paths(q, occs, float("nan"))
    with pytest.raises(KeyError):
        idx.paths(q, [o._replace(song="no such song")], PLANT_THETA)
    with pytest.raises(ValueError, match="leaves"):
        idx.paths(q[:o.q_rows[1]], [o], PLANT_THETA)                               # the last query row is not in fp
    with pytest.raises(ValueError, match="leaves"):
        idx.paths(q, [o._replace(r_rows=(o.r_rows[0], 90))], PLANT_THETA)          # "planted" has rows 0 .. 89
    with pytest.raises(ValueError, match="leaves"):
        idx.paths(q, [o._replace(q_rows=(o.q_rows[1], o.q_rows[0]))], PLANT_THETA)
    with pytest.raises(ValueError, match="leaves"):
        idx.paths(q, [o._replace(q_rows=(-1, o.q_rows[1]))], PLANT_THETA)
    with pytest.raises(TypeError):
        idx.paths(q, [(o.song, o.score)], PLANT_THETA)
    with pytest.raises(ValueError, match="row_hop_s"):
        idx.paths(q, occs, PLANT_THETA, row_hop_s=0.5)
    with pytest.raises(ValueError, match="d = 128"):
        idx.paths(q[:, :64].contiguous(), occs, PLANT_THETA)
    lidx, lq, _ = long_song
    big = Occurrence("long", 1.0, (0, ops.ALIGN_PATH_MAX), (0, ops.ALIGN_PATH_MAX), None, None, 1.0)
    fp = torch.zeros((ops.ALIGN_PATH_MAX + 4, 64), device=DEV)
    with pytest.raises(ValueError, match="limit"):
        lidx.paths(fp, [big], PLANT_THETA)
    with pytest.raises(ValueError, match="limit"):
        lidx.paths(fp, [big._replace(q_rows=(0, 5))], PLANT_THETA)
    assert ops.launch_counters() == before                             # nothing was launched for any of them
    # after the launch: these occurrences were not made from these rows with this threshold
    for bad in (o._replace(score=float(np.nextafter(np.float32(o.score), np.float32(np.inf)))),
                o._replace(q_rows=(o.q_rows[0] + 1, o.q_rows[1] + 1)), o._replace(r_rows=(o.r_rows[0], o.r_rows[1] - 1))):
        with pytest.raises(ValueError, match=r"occurrences\[1\]"):
            idx.paths(q, [occs[1], bad], PLANT_THETA)
    with pytest.raises(ValueError, match=r"occurrences\[0\]"):
        idx.paths(q, occs, PLANT_THETA + 0.01)
    assert ops.launch_counters()["align_paths"] == before["align_paths"] + 4
