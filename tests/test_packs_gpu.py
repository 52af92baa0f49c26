"""GPU: packs of songs of different lengths through the front ends in one launch (csrc/frontend.hip nsid_logmel_fft_ragged,
csrc/cqt.hip nsid_cqt_ragged), the ragged segment gather (csrc/misc.hip nsid_unfold_segments_ragged) and the database driver on
top of them (packs.py, fpdb.build_fp_db_from_waves).

The front-end and gather checks are bit-exact (torch.equal) against the batched entries on each song alone: the ragged kernels
share their arithmetic and differ in the work map only. The driver checks compare with extract_fingerprints on the same micro-batch
composition under the bound test_fingerprint_db_files uses (1e-5); the expected difference is 0 and the observed one is printed.
Every output buffer starts as NaN, so a column, row or segment nobody wrote cannot pass."""
import numpy as np
import pytest
import torch

from synth import GRAFP_CFG, synth_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGMEL_CFG = dict(GRAFP_CFG, fs=16000, n_fft=1024, win_len=1024, hop_len=512, overlap=0.875)
CQT_CFG = {"fs": 22050, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "arch": "resnet-ibn"}
# L: 513 legal minimum (T = 2, the reflections of both ends overlap); 4095 T = 8, one full run; 4096 T = 9, the second run holds one
# frame; 65023 T = 127, no segment; 65024 T = 128, S = 1; 73216 T = 144, S = 2 without a remainder; 100000 T = 196, S = 5
LOGMEL_LENGTHS = [513, 4095, 4096, 65023, 65024, 73216, 100000]
# 8193 legal minimum; 16383 T = 32, one full tile; 16384 T = 33; 110250 T = 216, S = 1; 130000 a longer song
CQT_LENGTHS = [8193, 16383, 16384, 110250, 130000]
SPARE = 5
_FRONTS = {}


def front_of(kind):
    from neuralsampleid_amd.frontend import CQTFrontEnd, LogMelFrontEnd
    if kind not in _FRONTS:
        _FRONTS[kind] = LogMelFrontEnd(LOGMEL_CFG, DEV) if kind == "logmel" else CQTFrontEnd(CQT_CFG, DEV)
    return _FRONTS[kind]


def noise(L, seed):
    return 0.1 * torch.randn(L, generator=torch.Generator().manual_seed(seed))


def counters(reset=False):
    from neuralsampleid_amd import _lib
    return _lib.launch_counters(reset=reset)


def build_pack(kind, waves, gap):
    """the waves as one pack (songs without a segment kept), its spectrogram buffer NaN before the launch"""
    from neuralsampleid_amd.packs import PackArena, WavePack, plan_pack
    front = front_of(kind)
    plan = plan_pack([w.numel() for w in waves], front, gap=gap, spare_cols=SPARE, require_segment=False)
    assert plan.n_songs == len(waves) and plan.ld == plan.total_cols + SPARE
    arena = PackArena(DEV)
    arena.spec(plan.n_rows * plan.ld).fill_(float("nan"))
    counters(reset=True)
    pack = WavePack(plan, waves, DEV, arena)
    c = counters()
    key = "logmel_fft_ragged" if kind == "logmel" else "cqt_ragged"
    assert c[key] == 1 and c["logmel_fft"] == 0 and c["cqt"] == 0, c          # ONE launch for the whole pack
    return pack


class Case:
    def __init__(self, kind, lengths, gap):
        self.kind = kind
        self.waves = [noise(L, 100 + j) for j, L in enumerate(lengths)]       # on the host: they travel through the staging buffer
        front = front_of(kind)
        self.alone = [front.batch(w.to(DEV)[None])[0].clone() for w in self.waves]          # each song in a launch of its own
        self.pack = build_pack(kind, self.waves, gap)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def logmel_case():
    return Case("logmel", LOGMEL_LENGTHS, 3)


@pytest.fixture(scope="module")
def cqt_case():
    return Case("cqt", CQT_LENGTHS, 1)


def check_front_end(case):
    plan, pack = case.pack.plan, case.pack
    assert any(int(o) % 2 for o in plan.offsets) and any(int(o) % 4 for o in plan.offsets)     # songs at odd sample offsets
    for j, want in enumerate(case.alone):
        got = pack.song_spec(j)
        assert got.shape == want.shape and bool(torch.isfinite(want).all()), j
        assert torch.equal(got, want), (j, int(plan.lengths[j]), float((got - want).abs().max()))
    assert plan.total_cols == sum(a.shape[1] for a in case.alone)
    assert bool(torch.isnan(pack.spec[:, plan.total_cols:]).all()) and pack.spec.shape[1] - plan.total_cols == SPARE
    # the same songs packed in reverse order (other offsets, other columns, other neighbours): the same per-song columns
    rev = build_pack(case.kind, case.waves[::-1], 2)
    n = len(case.waves)
    for j, want in enumerate(case.alone):
        assert torch.equal(rev.song_spec(n - 1 - j), want), j
    assert bool(torch.isnan(rev.spec[:, rev.plan.total_cols:]).all())


def test_logmel_pack_is_bit_equal_to_each_song_alone(logmel_case):
    assert [a.shape[1] for a in logmel_case.alone] == [2, 8, 9, 127, 128, 144, 196]
    assert logmel_case.pack.plan.segs.tolist() == [0, 0, 0, 0, 1, 2, 5]
    check_front_end(logmel_case)


def test_cqt_pack_is_bit_equal_to_each_song_alone(cqt_case):
    assert [a.shape[1] for a in cqt_case.alone] == [17, 32, 33, 216, 254]
    assert cqt_case.pack.plan.segs.tolist() == [0, 0, 0, 1, 1]
    check_front_end(cqt_case)


def test_songs_already_on_the_device(logmel_case):
    """songs on the GPU are copied into their slots there; mixed with host songs they give the same pack"""
    waves = [w.to(DEV) if j % 2 else w for j, w in enumerate(logmel_case.waves)]
    mixed = build_pack("logmel", waves, 3)
    assert torch.equal(mixed.spec[:, :mixed.plan.total_cols], logmel_case.pack.spec[:, :mixed.plan.total_cols])
    on_dev = build_pack("logmel", [w.to(DEV) for w in logmel_case.waves], 3)
    assert torch.equal(on_dev.spec[:, :mixed.plan.total_cols], logmel_case.pack.spec[:, :mixed.plan.total_cols])


@pytest.mark.parametrize("s0,nseg", [
    (4, 3),       # starts and ends inside the last song
    (0, 2),       # crosses one song boundary
    (0, 4),       # crosses two
    (2, 3),       # starts on a song's last segment
    (0, 8),       # the whole pack
    (0, 1), (2, 1), (7, 1),
])
def test_gather(logmel_case, s0, nseg):
    pack, plan = logmel_case.pack, logmel_case.pack.plan
    want = torch.cat([a.unfold(1, 128, 16).permute(1, 0, 2) for a in logmel_case.alone if a.shape[1] >= 128])
    assert want.shape == (8, 64, 128) and plan.total_segs == 8
    buf = torch.full((10, 64, 128), float("nan"), device=DEV)
    counters(reset=True)
    got = pack.segments(s0, nseg, buf)
    assert counters()["unfold_segments_ragged"] == 1
    assert got.shape == (nseg, 64, 128) and got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, want[s0:s0 + nseg])
    assert bool(torch.isnan(buf[nseg:]).all())
    with pytest.raises(RuntimeError):
        pack.segments(s0, 9 - s0, buf)                   # past the pack's last segment: refused on the host
    with pytest.raises(RuntimeError):
        pack.segments(s0, nseg, buf[:, :32])


def test_gather_cqt(cqt_case):
    pack = cqt_case.pack
    want = torch.cat([a.unfold(1, 216, 108).permute(1, 0, 2) for a in cqt_case.alone if a.shape[1] >= 216])
    buf = torch.full((3, 84, 216), float("nan"), device=DEV)
    assert torch.equal(pack.segments(0, 2, buf), want) and bool(torch.isnan(buf[2:]).all())


@pytest.fixture()
def fp32_modes():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    act, prec = F_.ACT_DTYPE, ops.get_gemm_precision()
    F_.set_activation_dtype(torch.float32)
    ops.set_gemm_precision("fp32")
    yield
    F_.set_activation_dtype(act)
    ops.set_gemm_precision(prec)


def gnn_model():
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    m = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"))
    m.load_state_dict(synth_state(m.state_dict()))
    return m.to(DEV).eval()


def check_driver(tmp_path, model, front, songs, want_segs, d, batch, pack_samples, want_packs, extract=None, tag="eager"):
    """both lookup styles; every pack's rows against extract_fingerprints on that pack's segments in the same micro-batches"""
    from neuralsampleid_amd import fpdb
    from neuralsampleid_amd.fingerprint import extract_fingerprints
    nf, step = front.n_frames, front.step
    out = {}
    for query_style in (False, True):
        root = str(tmp_path / f"{tag}_{int(query_style)}")
        counters(reset=True)
        n, dd, report = fpdb.build_fp_db_from_waves(model, front, iter(songs), root, "db", query_style=query_style, batch=batch,
                                                    pack_samples=pack_samples, extract=extract)
        c = counters()
        assert c["logmel_fft_ragged"] + c["cqt_ragged"] == len(want_packs) and c["logmel_fft"] == c["cqt"] == 0, c
        assert (n, dd) == (sum(want_segs), d)
        assert tuple(np.load(f"{root}/db_shape.npy")) == (n, d)
        lookup = []
        for idx, ((nm, _), s) in enumerate(zip(songs, want_segs)):
            lookup += [f"{nm}_{idx}" if query_style else nm] * s
        assert fpdb.load_lookup(root, "db") == lookup
        assert [(i, nm) for i, nm, _ in report["skipped"]] == [(i, nm) for i, ((nm, _), s) in enumerate(zip(songs, want_segs)) if s == 0]
        assert all(isinstance(r, str) and r for _, _, r in report["skipped"])
        assert [p["songs"] for p in report["packs"]] == want_packs
        data, shape = fpdb.load_memmap_data(root, "db")
        assert tuple(shape) == (n, d) and data.shape == (n, d)
        row, seen, worst = 0, [], 0.0
        for p in report["packs"]:
            lo, hi = p["songs"]
            segs = []
            for idx in range(lo, hi):
                seen.append(idx)
                spec = front.batch(songs[idx][1].to(DEV)[None])[0]
                if spec.shape[1] >= nf:
                    segs.append(spec.unfold(1, nf, step).permute(1, 0, 2))
            segs = torch.cat(segs).contiguous()
            assert p["rows"] == (row, row + segs.shape[0])
            want = extract_fingerprints(model, segs, batch=batch).cpu().numpy()
            worst = max(worst, float(np.abs(np.asarray(data[row:row + segs.shape[0]]) - want).max()))
            row += segs.shape[0]
        print(f"{tag} query_style={query_style}: max |driver - extract_fingerprints| = {worst:.3e}")
        assert seen == list(range(len(songs))) and row == n                  # no song left out of the comparison
        assert worst < 1e-5
        assert np.abs(np.linalg.norm(np.asarray(data), axis=1) - 1).max() < 1e-5
        out[query_style] = np.array(data)
    assert np.array_equal(out[False], out[True])
    return out[False]


# A: T = 160, S = 3; B: T = 128, S = 1; C: T = 59, too short for a segment; D: T = 196, S = 5; E: T = 144, S = 2.
# pack_samples = 150 000: A + B = 146 432 fit, C does not; C + D = 130 000 fit, E does not -> packs (A, B), (C, D), (E) of
# 4, 5 and 2 segments: with batch = 4 one full micro-batch, a full one plus a single segment, and a short one
GNN_SONGS = [("A", 81408), ("B", 65024), ("C", 30000), ("D", 100000), ("E", 73216)]
GNN_SEGS, GNN_PACKS = [3, 1, 0, 5, 2], [(0, 2), (2, 4), (4, 5)]


def gnn_songs():
    return [(nm, noise(L, 200 + j)) for j, (nm, L) in enumerate(GNN_SONGS)]


def test_driver_gnn(tmp_path, fp32_modes):
    check_driver(tmp_path, gnn_model(), front_of("logmel"), gnn_songs(), GNN_SEGS, 128, 4, 150000, GNN_PACKS)


def test_driver_baseline(tmp_path, fp32_modes):
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    model = BaselineModel(CQT_CFG, ResNetIBN())
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV).eval()
    songs = [("x", noise(110250 + 108 * 512, 301)), ("y", noise(110250, 302))]        # T = 324, S = 2 and T = 216, S = 1
    check_driver(tmp_path, model, front_of("cqt"), songs, [2, 1], 2048, 2, 1 << 26, [(0, 2)])


def test_driver_with_a_graphed_extractor(tmp_path, fp32_modes):
    from neuralsampleid_amd.fingerprint import GraphedFingerprinter
    model = gnn_model()
    songs = gnn_songs()
    eager = check_driver(tmp_path, model, front_of("logmel"), songs, GNN_SEGS, 128, 4, 150000, GNN_PACKS)
    graphed = check_driver(tmp_path, model, front_of("logmel"), songs, GNN_SEGS, 128, 4, 150000, GNN_PACKS,
                           extract=GraphedFingerprinter(model, micro_batch=4), tag="graphed")
    worst = float(np.abs(graphed - eager).max())
    print(f"max |graphed driver - eager driver| = {worst:.3e}")
    assert worst < 1e-5
