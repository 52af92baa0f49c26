"""GPU: the baseline's waveform effects (csrc/augment_fx.hip nsid_aug_compress / _biquad / _frames, modules/transformations.
GPUBaselineWaveAugment) against the oracle restatement (tests/baseline_augment_oracle.py), kernel by kernel and end to end, plus the
exact properties: batch independence, strided inputs, untouched rows, clamped parameters, capture, host-side refusals.

Compressor and frame edits: torch.equal with the oracle. Every operation of the compressor is one correctly rounded fp64 operation in
the stated order and the result is rounded to fp32 once; a frame edit moves float(float(gain * t1) + x_i), two fp32 operations.

Band EQ: metric max |y - y64| / max |y64| per clip, bound 2^-24 + 30 x FLOOR. FLOOR_EQ below is the same metric of the oracle in
np.longdouble against the oracle in fp64 on the same input, measured on the CPU per length as the worst clip of EQ_CASES (this
file's eq_floor() and eq_floor_train() print them); 30 is the headroom of tests/test_augment_gpu.py. Every input carries a noise floor, as there.

End to end the frame-edit clips are compared bit for bit, the vocoder clips under tests/test_augment_gpu.py's end-to-end bound for their
length plus the EQ term.

Measured on an MI355X (docs/experiments.md, "Baseline waveform augmentations on the GPU"; the tests print every figure): compressor and
frame edits 0 samples differ; band EQ 3.2e-8 .. 5.7e-8 per clip against the bound 5.96e-8 (the cascade is unfused and in the oracle's
order: what is left is the rounding to fp32); end to end EQ + stretch 1.5e-7 .. 5.9e-7, compressor + pitch 3.1e-7 .. 4.5e-7."""
import functools
import math

import numpy as np
import pytest
import torch

import baseline_augment_oracle as O
import test_augment_gpu as TA

pytestmark = pytest.mark.gpu
DEV = "cuda"
FS = 22050.0
CFG = {"arch": "resnet-ibn", "fs": 22050, "dur": 5.0, "gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5,
       "DC_threshold": [-30, 0], "DC_ratio": [2, 4, 8, 20], "DC_attack": [0.001, 0.1], "DC_release": [0.05, 1.0]}
LENGTHS = (1025, 3000, 8229)                          # one block and a bit, no multiple of 64 or 1024, more than eight blocks
S = 32
HEADROOM = 30.0
# np.longdouble oracle vs fp64 oracle, CPU: worst clip of EQ_CASES per length
FLOOR_EQ = {1025: 7.14e-13, 3000: 1.11e-12, 8229: 1.09e-12}
FLOOR_EQ_TRAIN = 1.39e-13                                # the two sampled clips of the B = 64, L = 110 250 batch
L_TRAIN, B_TRAIN = 110250, 64


def coef(t):
    return math.exp(-1.0 / (FS * t))


ATT_LO, ATT_HI, REL_LO, REL_HI = coef(0.001), coef(0.1), coef(0.05), coef(1.0)
# compressor clips: (peak the clip is scaled to, threshold, ratio, attack, release); None: a clip of another mode
CMP_CASES = {
    "b5": [(0.4, 0.5, 2.0, ATT_LO, REL_LO),           # threshold above the peak: identity
           (1.7, 1.0, 4.0, ATT_LO, REL_LO),           # threshold at 0 dB, the clip peaks above 1
           (0.9, 0.05, 8.0, ATT_HI, REL_HI),
           (0.9, 10 ** -1.5, 20.0, ATT_LO, REL_HI),
           None],
    "b1": [(0.6, 0.03, 2.0, ATT_HI, REL_LO)],
}
# frame clips at F = 8: (mode2, gain, frame_size as a fraction of L (None: past L), ops); None: a clip of another mode
F_TEST = 8
FRAME_CASES = {
    "b5": [(2, 1.0, 0.3, [0, 1, 0, 1]),               # 4 frames, the short last one doubled: longer than L
           (3, 1.0, 0.13, [0, 2, 2, 0, 0, 2, 0, 2]),  # 8 frames, the last short: shorter than L
           (4, 0.7, 0.21, [4, 0, 5, 0, 4]),           # silence, and silence + duplicate: two frames of zeros
           (2, 1.3, None, [1, 0, 0, 0, 0, 0, 0, 0]),  # frame_size >= L: one frame, doubled and cut
           None],
    "b1_duplicate": [(2, 1.0, 0.26, [1, 0, 1, 0])],
    "b1_remove": [(3, 1.0, 0.26, [2, 0, 0, 2])],      # the first and the short last frame dropped
    "b1_silence": [(4, 1.0, 0.26, [0, 4, 0, 4])],
}
# EQ clips: bands (order, centre Hz, bandwidth fraction, gain dB); [] with n_sec 0: identity
EQ_CASES = {
    "b6": [[(2, 1000.0, 0.5, -6.0)], [(3, 3000.0, 0.3, 4.0)], [(4, 500.0, 1.0, -20.0)],
           [(4, 700.0 + 150.0 * k, 1.0, 6.0 - k) for k in range(8)],           # 32 sections
           [(4, 50.0, 0.01, 10.0)],                                            # the 1 % band at 50 Hz
           []],
    "b1": [[(3, 8000.0, 1.0, 0.0), (2, 200.0, 0.2, 3.0)]],                     # a band clamped at Nyquist
}


def wave_n(n, seed, peak=None):
    """tones + a 0.05 noise floor at fs 22 050"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / FS
    x = 0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.1 * torch.sin(2 * math.pi * 3100.0 * t * (1 + 0.05 * t))
    x = (x + 0.05 * torch.randn(n, generator=g)).float()
    return x if peak is None else (x * (peak / float(x.abs().max()))).float()


def noise_n(n, seed):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def counters(reset=False):
    from neuralsampleid_amd import _lib
    return _lib.launch_counters(reset=reset)


NEW, OLD = ("aug_compress", "aug_biquad", "aug_frames"), ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish")


def module(**kw):
    from neuralsampleid_amd.modules.transformations import GPUBaselineWaveAugment
    kw.setdefault("generator", torch.Generator().manual_seed(11))
    return GPUBaselineWaveAugment(CFG, **kw)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def sentinel(B, L):
    return torch.full((B, L), 123.25, device=DEV)


# ---- compressor
@functools.lru_cache(maxsize=None)
def cmp_case(L, name):
    case = CMP_CASES[name]
    x = torch.stack([wave_n(L, 20 + b, c[0] if c else None) for b, c in enumerate(case)])
    mode1 = [1 if c else 2 for c in case]
    cmp = torch.tensor([c[1:] if c else (0.1, 2.0, 0.5, 0.5) for c in case], dtype=torch.float64)
    want = [torch.from_numpy(O.compress(x[b].numpy(), *c[1:])) if c else None for b, c in enumerate(case)]
    return x, mode1, cmp, want


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", list(CMP_CASES))
def test_compressor_equals_the_oracle(L, name):
    from neuralsampleid_amd import ops
    x, mode1, cmp, want = cmp_case(L, name)
    before = counters()
    out = ops.aug_compress(x.to(DEV), i32(mode1), cmp.to(DEV), sentinel(*x.shape)).cpu()
    assert counters()["aug_compress"] - before["aug_compress"] == 1
    for b, w in enumerate(want):
        if w is None:
            assert bool((out[b] == 123.25).all())
        else:
            print(f"compress {name} L={L} clip {b}: {int((out[b] != w).sum())} samples differ, peak in {float(x[b].abs().max()):.3f}, "
                  f"moved {int((w != x[b]).sum())}")
            assert torch.equal(out[b], w)
    if name == "b5":
        assert torch.equal(out[0], x[0]) and float(x[1].abs().max()) > 1.0 and not torch.equal(out[1], x[1])


# ---- frame edits
def frame_size_of(frac, L):
    return 10 ** 6 if frac is None else int(frac * L)


@functools.lru_cache(maxsize=None)
def frame_case(L, name):
    case = FRAME_CASES[name]
    B = len(case)
    x_i = torch.stack([noise_n(L, 60 + b) for b in range(B)])
    t1 = torch.stack([wave_n(L, 70 + b) for b in range(B)])
    mode2 = [c[0] if c else 1 for c in case]
    gain = torch.tensor([c[1] if c else 1.0 for c in case], dtype=torch.float32)
    fsz = [frame_size_of(c[2], L) if c else 100 for c in case]
    ops_ = torch.zeros(B, F_TEST, dtype=torch.int32)
    for b, c in enumerate(case):
        if c:
            ops_[b, :len(c[3])] = torch.tensor(c[3], dtype=torch.int32)
    want, lengths = [], []
    for b, c in enumerate(case):
        if not c:
            want.append(None)
            lengths.append(None)
            continue
        ed = O.frames(O.mix32(x_i[b].numpy(), t1[b].numpy(), gain[b].numpy()), O.clamp_frame_size(fsz[b], L, F_TEST), ops_[b].tolist())
        lengths.append(len(ed))
        want.append(torch.from_numpy(O.to_length(ed, L).astype(np.float32)))
    return x_i, t1, gain, mode2, fsz, ops_, want, lengths


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_frame_edits_equal_the_oracle(L, name):
    from neuralsampleid_amd import ops
    x_i, t1, gain, mode2, fsz, ops_, want, lengths = frame_case(L, name)
    before = counters()
    out = ops.aug_frames(x_i.to(DEV), t1.to(DEV), gain.to(DEV), i32(mode2), i32(fsz), ops_.to(DEV), sentinel(*x_i.shape)).cpu()
    assert counters()["aug_frames"] - before["aug_frames"] == 1
    for b, w in enumerate(want):
        if w is None:
            assert bool((out[b] == 123.25).all())
        else:
            print(f"frames {name} L={L} clip {b}: edited length {lengths[b]}, {int((out[b] != w).sum())} samples differ")
            assert torch.equal(out[b], w)
    if name == "b5":
        assert lengths[0] > L > lengths[1] and lengths[3] == 2 * L            # longer and shorter than L; one frame doubled
        assert all(int(f * L) and L % int(f * L) for _, _, f, _ in FRAME_CASES["b5"][:3])      # no frame size divides L
        assert bool((out[1, lengths[1]:] == 0).all()) and float(out[1, :lengths[1]].abs().max()) > 0


# ---- band EQ
def eq_table(bands):
    from neuralsampleid_amd.modules.transformations import butter_bandpass_sos
    tab = np.zeros((S, 6))
    tab[:, 0] = tab[:, 5] = 1.0
    secs = []
    for order, centre, frac, g in bands:
        bw = centre * frac
        secs.append((butter_bandpass_sos(order, centre - bw / 2, min(centre + bw / 2, 0.9999 * 0.5 * FS), FS), g))
    t = O.band_table(secs)
    tab[:len(t)] = t
    return tab, len(t)


@functools.lru_cache(maxsize=None)
def eq_case(L, name):
    case = EQ_CASES[name]
    x = torch.stack([wave_n(L, 40 + b) for b in range(len(case))])
    tabs = [eq_table(bands) for bands in case]
    sos = torch.from_numpy(np.stack([t for t, _ in tabs]))
    n_sec = [n for _, n in tabs]
    want = [O.cascade(x[b].numpy(), tabs[b][0][:n_sec[b]], np.float64) for b in range(len(case))]
    return x, sos, n_sec, want


def eq_floor(lengths=LENGTHS):
    """the figures of FLOOR_EQ: run on the CPU"""
    out = {}
    for L in lengths:
        worst = 0.0
        for name in EQ_CASES:
            x, sos, n_sec, want = eq_case(L, name)
            for b in range(len(want)):
                if n_sec[b]:
                    ext = O.cascade(x[b].numpy(), sos[b, :n_sec[b]].numpy(), np.longdouble)
                    worst = max(worst, float(np.abs(want[b] - ext).max() / np.abs(ext).max()))
        out[L] = worst
    return out


def eq_floor_train():
    _, _, x_j, p, eq, _, _ = train_batch()
    worst = 0.0
    for b in eq:
        tab = p.sos[b, :int(p.n_sec[b])].numpy()
        ext = O.cascade(x_j[b].numpy(), tab, np.longdouble)
        worst = max(worst, float(np.abs(O.cascade(x_j[b].numpy(), tab, np.float64) - ext).max() / np.abs(ext).max()))
    return worst


def eq_bound(floor):
    return 2.0 ** -24 + HEADROOM * floor


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", list(EQ_CASES))
def test_band_eq_against_the_oracle(L, name):
    from neuralsampleid_amd import ops
    x, sos, n_sec, want = eq_case(L, name)
    before = counters()
    out = ops.aug_biquad(x.to(DEV), i32([0] * len(want)), sos.to(DEV), i32(n_sec), sentinel(*x.shape)).cpu()
    assert counters()["aug_biquad"] - before["aug_biquad"] == 1
    errs = [O.rel(out[b].numpy(), w) for b, w in enumerate(want)]
    print(f"band EQ {name} L={L}: worst {max(errs):.3e} (per clip {' '.join(f'{e:.1e}' for e in errs)}), bound {eq_bound(FLOOR_EQ[L]):.3e}; "
          f"sections {n_sec}, output peaks {' '.join(f'{np.abs(w).max():.1e}' for w in want)}")
    assert bool(torch.isfinite(out).all())
    assert max(errs) <= eq_bound(FLOOR_EQ[L])
    if name == "b6":
        assert n_sec == [2, 3, 4, 32, 4, 0] and torch.equal(out[5], x[5])      # no section: the samples bit for bit


# ---- end to end: EQ + stretch, compressor + pitch, gain + each frame edit
def e2e_clips(L, m):
    F = m.frames_max(L)
    tab, n = eq_table([(3, 1200.0, 0.6, -3.0), (2, 4000.0, 0.4, 5.0)])
    ident = np.zeros((S, 6))
    ident[:, 0] = ident[:, 5] = 1.0
    base = {"gain": 1.0, "cmp": (0.1, 2.0, 0.5, 0.5), "sos": ident, "n_sec": 0, "rate": 1.0, "frame_size": 4410,
            "frame_ops": [0] * F}
    one = [1] + [0] * (F - 1)
    return [dict(base, mode1=0, sos=tab, n_sec=n, mode2=0, rate=np.float32(0.8)),
            dict(base, mode1=1, cmp=(0.05, 4.0, ATT_LO, REL_LO), mode2=1, rate=TA.A.pitch_rate(2)),
            dict(base, mode1=2, gain=1.9, mode2=2, frame_size=int(0.6 * L), frame_ops=one),
            dict(base, mode1=2, gain=0.45, mode2=3, frame_size=int(0.6 * L), frame_ops=[2 * v for v in one]),
            dict(base, mode1=2, gain=1.2, mode2=4, frame_size=int(0.6 * L), frame_ops=[4 * v for v in one])]


def params_of(clips, dev=DEV):
    from neuralsampleid_amd.modules.transformations import BaselineAugmentParams

    def col(k, dt):
        return torch.tensor(np.array([c[k] for c in clips]), dtype=dt).to(dev)
    return BaselineAugmentParams(col("mode1", torch.int32), col("gain", torch.float32), col("cmp", torch.float64), col("sos", torch.float64),
                                 col("n_sec", torch.int32), col("mode2", torch.int32), col("rate", torch.float32),
                                 col("frame_size", torch.int32), col("frame_ops", torch.int32))


@functools.lru_cache(maxsize=None)
def e2e_inputs(L, B=5):
    return torch.stack([noise_n(L, 80 + b) for b in range(B)]), torch.stack([wave_n(L, 90 + b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def e2e_reference(L):
    x_i, x_j = e2e_inputs(L)
    return [O.augment(x_i[b].numpy(), x_j[b].numpy(), c) for b, c in enumerate(e2e_clips(L, module()))]


@pytest.mark.parametrize("L", LENGTHS)
def test_forward_end_to_end(L):
    m = module()
    x_i, x_j = e2e_inputs(L)
    want = e2e_reference(L)
    xj = x_j.to(DEV)
    before = counters()
    out, same = m(x_i.to(DEV), xj, params_of(e2e_clips(L, m)))
    after = counters()
    assert same is xj and out.shape == (5, L) and out.dtype == torch.float32
    assert all(after[k] - before[k] == 1 for k in NEW + OLD)
    out = out.cpu()
    bound = TA.HEADROOM * TA.FLOOR[L]["e2e"]
    errs = [O.rel(out[b].numpy(), want[b]) for b in range(2)]
    print(f"forward L={L}: EQ + stretch {errs[0]:.3e} (bound {bound + eq_bound(FLOOR_EQ[L]):.3e}), compressor + pitch {errs[1]:.3e} "
          f"(bound {bound:.3e}); frame clips differ in {[int((out[b].numpy() != want[b]).sum()) for b in (2, 3, 4)]} samples")
    assert bool(torch.isfinite(out).all())
    assert errs[0] <= bound + eq_bound(FLOOR_EQ[L]) and errs[1] <= bound
    for b in (2, 3, 4):
        assert np.array_equal(out[b].numpy().astype(np.float64), want[b])


@pytest.mark.parametrize("which", ["eq_stretch", "compress_pitch", "gain_duplicate", "gain_remove", "gain_silence"])
def test_forward_one_clip_per_mode(which):
    """B = 1: the clip alone equals the clip in the batch of five, bit for bit"""
    L, m = 3000, module()
    b = ["eq_stretch", "compress_pitch", "gain_duplicate", "gain_remove", "gain_silence"].index(which)
    x_i, x_j = e2e_inputs(L)
    clips = e2e_clips(L, m)
    whole = m(x_i.to(DEV), x_j.to(DEV), params_of(clips))[0]
    alone = m(x_i[b:b + 1].to(DEV), x_j[b:b + 1].to(DEV), params_of(clips[b:b + 1]))[0]
    assert torch.equal(alone[0], whole[b])
    assert torch.equal(m(x_i.to(DEV), x_j.to(DEV), params_of(clips))[0], whole)


# ---- one batch of the workload's size
@functools.lru_cache(maxsize=None)
def train_batch():
    m = module()
    m.num_bands, m.band_gains_db = 2, [-4.0, 6.0]                                # at most 8 sections per clip
    g = torch.Generator().manual_seed(1)
    x_i = 0.1 * torch.randn(B_TRAIN, L_TRAIN, generator=g)
    x_j = 0.1 * torch.randn(B_TRAIN, L_TRAIN, generator=g)
    p = m.draw(B_TRAIN, generator=torch.Generator().manual_seed(2), device="cpu", L=L_TRAIN)
    eq = [int(b) for b in torch.nonzero(p.mode1 == 0)[:2, 0]]
    cm = [int(b) for b in torch.nonzero(p.mode1 == 1)[:2, 0]]
    fr = [int(b) for b in torch.nonzero((p.mode2 >= 2) & (p.mode1 == 2))[:2, 0]]
    for b in eq + cm + fr:
        x_j[b] = wave_n(L_TRAIN, 200 + b, 1.5)                                    # above every threshold of the range
    return m, x_i, x_j, p, eq, cm, fr


def clip_of(p, b):
    return {k: getattr(p, k)[b].numpy() for k in p._fields}


def test_training_batch():
    """B = 64 clips of 5 s with drawn parameters: every row finite, two sampled clips per new kernel against the oracle (the T1 kernels'
    rows are read from the module's workspace); the new kernels once, the four of the vocoder chain once per chunk of 64"""
    m, x_i, x_j, p, eq, cm, fr = train_batch()
    assert len(eq) == len(cm) == len(fr) == 2
    from neuralsampleid_amd.modules.transformations import BaselineAugmentParams
    before = counters()
    out, _ = m(x_i.to(DEV), x_j.to(DEV), BaselineAugmentParams(*(t.to(DEV) for t in p)))
    after = counters()
    assert all(after[k] - before[k] == 1 for k in NEW + OLD)
    t1 = next(iter(m._ws.values()))["t1"].cpu()
    out = out.cpu()
    assert out.shape == (B_TRAIN, L_TRAIN) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(t1).all())
    for b in cm:
        want = O.compress(x_j[b].numpy(), *p.cmp[b].tolist())
        assert int((want != x_j[b].numpy()).sum()) > 1000 and torch.equal(t1[b], torch.from_numpy(want))
    for b in fr:
        assert np.array_equal(out[b].numpy().astype(np.float64), O.augment(x_i[b].numpy(), x_j[b].numpy(), clip_of(p, b)))
    for b in eq:
        n = int(p.n_sec[b])
        assert 4 <= n <= 8
        err = O.rel(t1[b].numpy(), O.cascade(x_j[b].numpy(), p.sos[b, :n].numpy(), np.float64))
        print(f"training batch: EQ clip {b}, {n} sections: {err:.3e}, bound {eq_bound(FLOOR_EQ_TRAIN):.3e}")
        assert err <= eq_bound(FLOOR_EQ_TRAIN)
    others = [b for b in range(B_TRAIN) if int(p.mode1[b]) == 2]
    assert torch.equal(t1[others], x_j[others])


# ---- exact properties
def test_a_clip_does_not_depend_on_its_batch():
    from neuralsampleid_amd import ops
    L = 3000
    x, mode1, cmp, _ = cmp_case(L, "b5")
    xd, cd = x.to(DEV), cmp.to(DEV)
    a = ops.aug_compress(xd, i32(mode1), cd, sentinel(5, L))
    for b in range(4):
        assert torch.equal(ops.aug_compress(xd[b:b + 1].clone(), i32(mode1[b:b + 1]), cd[b:b + 1].clone())[0], a[b])
    x, sos, n_sec, _ = eq_case(L, "b6")
    xd, sd = x.to(DEV), sos.to(DEV)
    a = ops.aug_biquad(xd, i32([0] * 6), sd, i32(n_sec))
    for b in range(6):
        assert torch.equal(ops.aug_biquad(xd[b:b + 1].clone(), i32([0]), sd[b:b + 1].clone(), i32(n_sec[b:b + 1]))[0], a[b])
    x_i, t1, gain, mode2, fsz, ops_, _, _ = frame_case(L, "b5")
    args = (x_i.to(DEV), t1.to(DEV), gain.to(DEV), i32(mode2), i32(fsz), ops_.to(DEV))
    a = ops.aug_frames(*args, sentinel(5, L))
    for b in range(4):
        assert torch.equal(ops.aug_frames(*(t[b:b + 1].clone() for t in args))[0], a[b])


def test_strided_views_equal_contiguous_input():
    L, m = 3000, module()
    x_i, x_j = e2e_inputs(L)
    p = params_of(e2e_clips(L, m))
    want = m(x_i.to(DEV), x_j.to(DEV), p)[0]
    views = []
    for x in (x_i, x_j):
        big = torch.full((5 * (L + 107) + 3,), float("nan"), device=DEV)
        v = big[3:].view(5, L + 107)[:, :L]                                   # odd first offset, NaN in the gaps
        v.copy_(x)
        assert v.stride(0) == L + 107 and v.storage_offset() == 3
        views.append(v)
    got = m(views[0], views[1], p)[0]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_clips_of_another_mode_are_untouched():
    """every new kernel, every mode that is not its own: the sentinel stays"""
    from neuralsampleid_amd import ops
    L, B = 3000, 6
    x = torch.stack([wave_n(L, 30 + b) for b in range(B)]).to(DEV)
    cmp = torch.tensor([(0.05, 4.0, ATT_LO, REL_LO)] * B, dtype=torch.float64, device=DEV)
    _, sos, _, _ = eq_case(L, "b6")
    sos = sos.to(DEV)
    out = ops.aug_compress(x, i32([1, 0, 2, -1, 7, 1]), cmp, sentinel(B, L))
    assert bool((out[1:5] == 123.25).all()) and not bool((out[0] == 123.25).any()) and not bool((out[5] == 123.25).any())
    out = ops.aug_biquad(x, i32([0, 1, 2, -1, 7, 0]), sos, i32([2] * B), sentinel(B, L))
    assert bool((out[1:5] == 123.25).all()) and not bool((out[0] == 123.25).all()) and not bool((out[5] == 123.25).all())
    fo = torch.zeros(B, F_TEST, dtype=torch.int32, device=DEV)
    out = ops.aug_frames(x, x, torch.ones(B, device=DEV), i32([2, 0, 1, -1, 5, 4]), i32([1000] * B), fo, sentinel(B, L))
    assert bool((out[1:5] == 123.25).all()) and torch.equal(out[0], x[0] + x[0]) and torch.equal(out[5], x[5] + x[5])


def test_parameters_outside_their_ranges_are_clamped():
    """mode1 outside {0, 1} is the gain option, mode2 outside 1 .. 4 the time stretch; n_sec is clamped into [0, S], frame_size into
    [ceil(L / F), L]; compressor parameters to threshold >= 0, ratio >= 1, attack / release in [0, 1] with NaN at the lower end: the
    result is the clamped clip's"""
    from neuralsampleid_amd import ops
    L, m = 3000, module()
    x_i, x_j = e2e_inputs(L)
    xi, xj = x_i.to(DEV), x_j.to(DEV)
    clips = e2e_clips(L, m)
    F = m.frames_max(L)
    odd = [dict(clips[0], n_sec=99), dict(clips[1], cmp=(float("nan"), 0.5, float("nan"), 7.0)), dict(clips[2], frame_size=0),
           dict(clips[3], frame_size=10 ** 9), dict(clips[4], mode1=-5, mode2=9, rate=np.float32(1.1))]
    clamped = [dict(clips[0], n_sec=S), dict(clips[1], cmp=(0.0, 1.0, 0.0, 1.0)), dict(clips[2], frame_size=-(-L // F)),
               dict(clips[3], frame_size=L), dict(clips[4], mode1=2, mode2=0, rate=np.float32(1.1))]
    got, want = m(xi, xj, params_of(odd))[0], m(xi, xj, params_of(clamped))[0]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    x, sos, n_sec, _ = eq_case(L, "b6")
    a = ops.aug_biquad(x.to(DEV), i32([0] * 6), sos.to(DEV), i32([-3, 3, 4, 99, 4, 0]))
    b = ops.aug_biquad(x.to(DEV), i32([0] * 6), sos.to(DEV), i32([0, 3, 4, S, 4, 0]))
    assert torch.equal(a, b) and torch.equal(a[0], x[0].to(DEV))
    # the clamped compressor clip against the oracle: ratio 1, release 1 holds g at 1 below and moves it nowhere above
    c = ops.aug_compress(xj[1:2], i32([1]), torch.tensor([[float("nan"), 0.5, float("nan"), 7.0]], dtype=torch.float64, device=DEV))
    assert torch.equal(c[0].cpu(), torch.from_numpy(O.compress(x_j[1].numpy(), *O.clamp_cmp((float("nan"), 0.5, float("nan"), 7.0)))))


def test_forward_is_capturable():
    """one stream, torch.cuda.graph; replay after the inputs and every parameter tensor changed in place = eager on the new contents"""
    L, m = 3000, module()
    x_i, x_j = e2e_inputs(L)
    xi, xj = x_i.to(DEV).clone(), x_j.to(DEV).clone()
    clips = e2e_clips(L, m)
    p = params_of(clips)
    m(xi, xj, p)                                                              # tables and workspaces exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    counters(reset=True)
    with torch.cuda.graph(graph):
        out, _ = m(xi, xj, p)
    cap = counters()
    assert all(cap[k] == 1 for k in NEW + OLD) and sum(cap.values()) == 7
    xi.copy_(x_j.to(DEV) * 0.5)
    xj.copy_(x_i.to(DEV) + 0.7 * x_j.to(DEV))
    q = params_of([dict(clips[(b + 2) % 5], gain=0.8 + 0.1 * b) for b in range(5)])
    for dst, src in zip(p, q):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = m(xi, xj, p)[0]
    assert torch.equal(out, eager) and not torch.equal(eager[0], eager[1])


def test_no_transform_options():
    """max_transforms_1 = 0: T1 is the identity whatever the draw says; max_transforms_2 = 0: rate 1 and no frame edit"""
    L = 3000
    x_i, x_j = e2e_inputs(L)
    m = module(max_transforms_1=0, max_transforms_2=0)
    out, _ = m(torch.zeros(5, L, device=DEV), x_j.to(DEV), params_of(e2e_clips(L, m)))
    errs = [O.rel(out[b].cpu().numpy(), x_j[b].numpy().astype(np.float64)) for b in range(5)]
    print(f"identity: {max(errs):.3e}")
    assert max(errs) <= TA.HEADROOM * TA.FLOOR[L]["e2e"]
    m = module(max_transforms_1=0)
    clips = e2e_clips(L, m)
    got = m(x_i.to(DEV), x_j.to(DEV), params_of(clips))[0]
    want = m(x_i.to(DEV), x_j.to(DEV), params_of([dict(c, mode1=2, gain=1.0) for c in clips]))[0]
    assert torch.equal(got, want)


def test_host_checks_launch_nothing():
    from neuralsampleid_amd import _lib, ops
    L, B = 3000, 2
    x, out = torch.zeros(B, L, device=DEV), torch.zeros(B, L, device=DEV)
    mode, gain = torch.zeros(B, dtype=torch.int32, device=DEV), torch.ones(B, device=DEV)
    cmp = torch.ones(B, 4, dtype=torch.float64, device=DEV)
    sos = torch.ones(B, S, 6, dtype=torch.float64, device=DEV)
    fo = torch.zeros(B, F_TEST, dtype=torch.int32, device=DEV)
    P, lib, s = ops._p, _lib.lib, ops._stream()
    counters(reset=True)
    bad = [
        lib.nsid_aug_compress(P(x), L, B, 0, P(mode), P(cmp), P(out), L, s),                                   # L < 1
        lib.nsid_aug_compress(P(x), L, B, 1 << 30, P(mode), P(cmp), P(out), L, s),                             # L >= 2^30
        lib.nsid_aug_compress(P(x), L - 1, B, L, P(mode), P(cmp), P(out), L, s),                               # stride shorter than a row
        lib.nsid_aug_compress(P(x), L, B, L, P(mode), P(cmp), P(out), L - 1, s),
        lib.nsid_aug_compress(P(x), L, 0, L, P(mode), P(cmp), P(out), L, s),                                   # B < 1
        lib.nsid_aug_compress(P(x), L, B, L, P(mode), P(cmp) + 4, P(out), L, s),                               # misaligned doubles
        lib.nsid_aug_compress(P(x), L, B, L, None, P(cmp), P(out), L, s),                                      # null
        lib.nsid_aug_biquad(P(x), L, B, L, P(mode), P(sos), 0, P(mode), P(out), L, s),                         # S < 1
        lib.nsid_aug_biquad(P(x), L, B, L, P(mode), P(sos), 65, P(mode), P(out), L, s),                        # S > 64
        lib.nsid_aug_biquad(P(x), L, B, L, P(mode), P(sos) + 4, S, P(mode), P(out), L, s),
        lib.nsid_aug_biquad(P(x), L, B, L, P(mode), P(sos), S, None, P(out), L, s),
        lib.nsid_aug_biquad(P(x), L, B, L, P(mode), P(sos), S, P(mode), P(out), L - 1, s),
        lib.nsid_aug_biquad(P(x), L, B, 0, P(mode), P(sos), S, P(mode), P(out), L, s),
        lib.nsid_aug_frames(P(x), L, P(x), L, P(gain), B, L, P(mode), P(mode), P(fo), 0, P(out), L, s),        # F < 1
        lib.nsid_aug_frames(P(x), L, P(x), L, P(gain), B, L, P(mode), P(mode), P(fo), 257, P(out), L, s),      # F > 256
        lib.nsid_aug_frames(P(x), L, P(x), L - 1, P(gain), B, L, P(mode), P(mode), P(fo), F_TEST, P(out), L, s),
        lib.nsid_aug_frames(P(x), L, P(x), L, P(gain), 65536, L, P(mode), P(mode), P(fo), F_TEST, P(out), L, s),
        lib.nsid_aug_frames(P(x), L, P(x), L, None, B, L, P(mode), P(mode), P(fo), F_TEST, P(out), L, s),
        lib.nsid_aug_frames(P(x), L, P(x), L, P(gain), B, 1 << 30, P(mode), P(mode), P(fo), F_TEST, P(out), L, s),
    ]
    assert bad == [-1] * len(bad)
    assert sum(counters().values()) == 0
    torch.cuda.synchronize()
