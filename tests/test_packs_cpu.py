"""CPU: the host side of the packed database build (neuralsampleid_amd/packs.py, fpdb.build_fp_db_from_waves) — the planner against
plain loops, its refusals, the bindings of the three ragged entry points and the append writer. No GPU."""
import dataclasses
import filecmp

import numpy as np
import pytest
import torch

LOGMEL_CFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875,
              "arch": "grafp"}
CQT_CFG = {"fs": 22050, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "arch": "resnet-ibn"}
_FRONTS = {}


def front_of(kind):
    from neuralsampleid_amd.frontend import CQTFrontEnd, LogMelFrontEnd
    if kind not in _FRONTS:
        _FRONTS[kind] = LogMelFrontEnd(LOGMEL_CFG, "cpu", stft="fft") if kind == "logmel" else CQTFrontEnd(CQT_CFG, "cpu")
    return _FRONTS[kind]


def brute_segments(T, n_frames, step):
    """the row count of the reference's unfold (transformations.py:101-104), 0 where it raises"""
    try:
        return torch.zeros(T, 1).unfold(0, n_frames, step).shape[0]
    except RuntimeError:
        return 0


LENGTHS = {
    # around the reflect minimum, the run of 8 frames, one segment, a segment boundary, and a long song
    "logmel": [513, 4095, 4096, 65023, 65024, 73215, 73216, 100000, 480000, 512, 1],
    # the same around width/2 = 8192, the tile of 32 frames and the 216-frame segment (step 108)
    "cqt": [8193, 16383, 16384, 110080, 110591, 110592, 165887, 165888, 130000, 661500, 8192, 100],
}


@pytest.mark.parametrize("kind", ["logmel", "cqt"])
@pytest.mark.parametrize("require_segment,gap,spare", [(True, 0, 0), (False, 3, 5)])
def test_plan_against_plain_loops(kind, require_segment, gap, spare):
    from neuralsampleid_amd.packs import plan_pack
    front = front_of(kind)
    hop, nf, step = front.hop, front.n_frames, front.step
    min_len = 512 if kind == "logmel" else 8192
    item = 8 if kind == "logmel" else 32
    assert (nf, step) == ((128, 16) if kind == "logmel" else (216, 108))
    lengths = LENGTHS[kind]
    plan = plan_pack(lengths, front, gap=gap, spare_cols=spare, require_segment=require_segment)
    off = col = items = seg = 0
    index, table, seg_col, seg_start, S_all, skipped = [], [], [], [], [], []
    for j, L in enumerate(lengths):
        T = 1 + L // hop
        S = brute_segments(T, nf, step)
        if L <= min_len or (require_segment and S == 0):
            skipped.append(j)
            continue
        index.append(j)
        table.append((off, L, col, items))
        seg_start.append(seg)
        S_all.append(S)
        seg_col.extend(col + k * step for k in range(S))
        off, col, items, seg = off + L + gap, col + T, items + -(-T // item), seg + S
    assert [j for j, _ in plan.skipped] == skipped and all(isinstance(r, str) and r for _, r in plan.skipped)
    assert plan.index.tolist() == index and plan.segs.tolist() == S_all
    assert plan.table().tolist() == [list(r) for r in table] and plan.table().dtype == np.int64
    assert plan.seg_col.tolist() == seg_col and plan.seg_start.tolist() == seg_start + [seg]
    assert plan.total_cols == col and plan.ld == col + spare and plan.total_items == items and plan.total_segs == seg
    assert plan.total_samples == off - gap and plan.max_len == max(lengths[j] for j in index)
    assert plan.n_rows == (64 if kind == "logmel" else 84)
    assert any(s == 0 for s in S_all) == (not require_segment)        # the case list reaches the segment-less branch
    plan.validate()


def test_short_songs_are_excluded_and_reported():
    from neuralsampleid_amd.packs import plan_pack
    front = front_of("logmel")
    plan = plan_pack([512, 513, 70000, 0], front)
    assert plan.index.tolist() == [2] and [j for j, _ in plan.skipped] == [0, 1, 3]
    assert "reflect" in plan.skipped[0][1] and "segment" in plan.skipped[1][1] and "reflect" in plan.skipped[2][1]
    kept = plan_pack([512, 513, 70000], front, require_segment=False)
    assert kept.index.tolist() == [1, 2] and [j for j, _ in kept.skipped] == [0]
    empty = plan_pack([512, 100], front)
    assert empty.n_songs == 0 and empty.total_segs == 0 and len(empty.skipped) == 2
    with pytest.raises(ValueError):
        empty.validate()
    cq = plan_pack([8192, 8193, 110250], front_of("cqt"))
    assert cq.index.tolist() == [2] and [j for j, _ in cq.skipped] == [0, 1]


def test_oversized_packs_raise():
    from neuralsampleid_amd.packs import plan_pack
    with pytest.raises(ValueError, match="2\\^30"):
        plan_pack([1 << 29, 1 << 29], front_of("logmel"))
    with pytest.raises(ValueError, match="2\\^30"):
        plan_pack([(1 << 30) + 7], front_of("logmel"))
    plan_pack([(1 << 29) - 1, 1 << 29], front_of("logmel"))            # 2^30 - 1 samples: the largest pack
    with pytest.raises(ValueError, match="2\\^28"):
        plan_pack([1 << 28], front_of("cqt"))
    with pytest.raises(TypeError):
        plan_pack([70000], object())


def test_waves_are_checked_before_anything_is_uploaded():
    from neuralsampleid_amd.packs import WavePack, check_wave, plan_pack
    front = front_of("logmel")
    plan = plan_pack([70000], front)
    check_wave(torch.zeros(70000), 70000)
    for bad in (torch.zeros(1, 70000), torch.zeros(70000, dtype=torch.float64), torch.zeros(70000, dtype=torch.int16),
                np.zeros(70000, np.float32)):
        with pytest.raises(TypeError):
            check_wave(bad)
        with pytest.raises(TypeError):
            WavePack(plan, [bad], "cpu")
    with pytest.raises(ValueError):
        WavePack(plan, [torch.zeros(70001)], "cpu")              # not the planned length
    with pytest.raises(ValueError):
        WavePack(plan, [], "cpu")
    with pytest.raises(TypeError):
        WavePack(object(), [torch.zeros(70000)], "cpu")
    with pytest.raises(ValueError):
        WavePack(dataclasses.replace(plan, front=front_of("cqt")), [torch.zeros(70000)], "cpu")    # a plan that is not its front end's


def test_corrupted_tables_fail_validation():
    from neuralsampleid_amd.packs import plan_pack
    plan = plan_pack([70000, 100000, 65024], front_of("logmel"), spare_cols=2)
    with pytest.raises(ValueError):
        plan.cols[1] += 1                                               # the planner's arrays are read-only
    for name, where, delta in (("cols", 1, 1), ("offsets", 2, -1), ("prefix", 1, -1), ("frames", 0, 1), ("segs", 0, 1),
                               ("seg_col", -1, 1), ("seg_start", 1, 1), ("lengths", 0, 512), ("lengths", 2, -64600)):
        a = getattr(plan, name).copy()
        a[where] += delta
        with pytest.raises(ValueError):
            dataclasses.replace(plan, **{name: a}).validate()
    with pytest.raises(ValueError):
        dataclasses.replace(plan, ld=plan.total_cols - 1).validate()
    with pytest.raises(ValueError):
        dataclasses.replace(plan, seg_col=plan.seg_col[:-1].copy()).validate()
    with pytest.raises(ValueError):
        dataclasses.replace(plan, seg_col=plan.seg_col.astype(np.int32)).validate()
    with pytest.raises(ValueError):
        dataclasses.replace(plan, item=32).validate()
    dataclasses.replace(plan, ld=plan.total_cols).validate()


def test_entry_points_are_bound_and_refuse_before_any_launch():
    """null pointers and every bad scalar: NSID_EINVAL = -1 on the host, nothing launched, nothing counted (the arguments below are
    never dereferenced: every refusal comes before the launch, and the good-scalar call has null pointers)"""
    from neuralsampleid_amd import _lib
    names = ("nsid_logmel_fft_ragged", "nsid_cqt_ragged", "nsid_unfold_segments_ragged")
    assert all(n in _lib.EXPORTS and hasattr(_lib.lib, n) for n in names)
    assert _lib.SIGNATURES["nsid_logmel_fft_ragged"] == "ppillliippppipls"
    assert _lib.SIGNATURES["nsid_cqt_ragged"] == "ppillliiipiplppls"
    assert _lib.SIGNATURES["nsid_unfold_segments_ragged"] == "pliiplips"
    keys = ("logmel_fft_ragged", "cqt_ragged", "unfold_segments_ragged")
    _lib.launch_counters(reset=True)
    P = 1 << 20                                                          # a non-null "pointer": 16-byte aligned, never read
    lm = _lib.lib.nsid_logmel_fft_ragged
    good = dict(pack=P, songs=P, n=2, max_len=70000, runs=40, cols=300, n_fft=1024, hop=512, win=P, tw=P, fb=P, band=P, mels=64,
                out=P, ld=300)
    def call_lm(**kw):
        a = dict(good, **kw)
        return lm(a["pack"], a["songs"], a["n"], a["max_len"], a["runs"], a["cols"], a["n_fft"], a["hop"], a["win"], a["tw"],
                  a["fb"], a["band"], a["mels"], a["out"], a["ld"], None)
    for ptr in ("pack", "songs", "win", "tw", "fb", "band", "out"):
        assert call_lm(**{ptr: None}) == -1, ptr
    for bad in (dict(n=0), dict(n_fft=512), dict(n_fft=2048), dict(hop=0), dict(hop=1025), dict(mels=0), dict(max_len=512),
                dict(max_len=1 << 30), dict(ld=299), dict(cols=0), dict(runs=1 << 31), dict(runs=1), dict(tw=P + 4)):
        assert call_lm(**bad) == -1, bad
    front = front_of("cqt")
    groups = front.groups
    cq = _lib.lib.nsid_cqt_ragged
    goodc = dict(pack=P, songs=P, n=2, max_len=130000, tiles=12, cols=300, hop=512, width=16384, bins=84, groups=groups.ctypes.data,
                 ng=groups.shape[0], taps=P, taps_len=front.taps.numel(), scale=P, out=P, ld=300)
    def call_cq(**kw):
        a = dict(goodc, **kw)
        return cq(a["pack"], a["songs"], a["n"], a["max_len"], a["tiles"], a["cols"], a["hop"], a["width"], a["bins"], a["groups"],
                  a["ng"], a["taps"], a["taps_len"], a["scale"], a["out"], a["ld"], None)
    for ptr in ("pack", "songs", "groups", "taps", "scale", "out"):
        assert call_cq(**{ptr: None}) == -1, ptr
    for bad in (dict(n=0), dict(hop=0), dict(hop=64), dict(width=16383), dict(width=0), dict(bins=83), dict(ng=0), dict(ng=33),
                dict(max_len=8192), dict(max_len=1 << 28), dict(ld=299), dict(cols=0), dict(tiles=1 << 31), dict(tiles=1),
                dict(tiles=(1 << 31) // groups.shape[0] + 1), dict(taps=P + 4), dict(taps_len=front.taps.numel() - 1)):
        assert call_cq(**bad) == -1, bad
    uf = _lib.lib.nsid_unfold_segments_ragged
    assert uf(None, 300, 64, 128, P, 0, 4, P, None) == -1
    assert uf(P, 300, 64, 128, None, 0, 4, P, None) == -1
    assert uf(P, 300, 64, 128, P, 0, 4, None, None) == -1
    for ld, rows, nf, s0, nseg in ((127, 64, 128, 0, 4), (300, 0, 128, 0, 4), (300, 64, 0, 0, 4), (300, 64, 128, -1, 4),
                                   (300, 64, 128, 0, 0), (300, 64, 128, 0, -3)):
        assert uf(P, ld, rows, nf, P, s0, nseg, P, None) == -1, (ld, rows, nf, s0, nseg)
    c = _lib.launch_counters()
    assert all(c[k] == 0 for k in keys), {k: c[k] for k in keys}


def test_append_writer_is_byte_identical_to_write_fp_db(tmp_path):
    from neuralsampleid_amd import fpdb
    rows = np.random.default_rng(3).standard_normal((11, 128)).astype(np.float32)
    rows[2, 5] = np.nan
    names = ["a"] * 4 + ["b_1"] + ["c é"] * 6
    assert fpdb.write_fp_db(str(tmp_path / "one"), "db", rows, names) == (11, 128)
    w = fpdb.FpDbAppender(str(tmp_path / "two"), "db", 128)
    w.append(rows[:4], names[:4])
    w.append(torch.from_numpy(rows[4:5]), names[4:5])
    w.append(rows[5:5], [])
    w.append(rows[5:], names[5:])
    with pytest.raises(ValueError):
        w.append(rows[:2], ["x"])
    with pytest.raises(ValueError):
        w.append(rows[:2, :64], ["x", "y"])
    assert w.close() == (11, 128)
    for f in ("db.mm", "db_shape.npy", "db_lookup.json"):
        assert filecmp.cmp(str(tmp_path / "one" / f), str(tmp_path / "two" / f), shallow=False), f
    data, shape = fpdb.load_memmap_data(str(tmp_path / "two"), "db")
    assert tuple(shape) == (11, 128) and fpdb.load_lookup(str(tmp_path / "two"), "db") == names


def test_driver_signature():
    import inspect
    from neuralsampleid_amd import fpdb
    sig = inspect.signature(fpdb.build_fp_db_from_waves)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("model", inspect.Parameter.empty), ("front", inspect.Parameter.empty), ("songs", inspect.Parameter.empty),
        ("output_root_dir", inspect.Parameter.empty), ("fname", "ref_db"), ("query_style", False), ("batch", 1024),
        ("pack_samples", 1 << 26), ("extract", None)]
