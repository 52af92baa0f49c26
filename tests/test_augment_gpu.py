"""GPU: the waveform augmentations (csrc/augment.hip nsid_aug_stft / _vocoder / _istft / _finish, modules/transformations.
GPUWaveAugment) against the fp64 oracle restatement (tests/augment_oracle.py), stage by stage and end to end, plus the exact
properties: batch independence, strided inputs, clamped parameters, zero tails, capture, host-side refusals.

Metric: max |y - y64| / max |y64| per clip. Bound: 30 x the same metric of the oracle's own fp32 mode (real fp32 FFTs, fp32 wrapped
phase sum, fp32 dot products) against fp64 on the same input, the headroom tests/test_frontend_batch_gpu.py documents for its dB
bound. FLOOR below is that fp32 floor, measured on the CPU per length and stage as the worst of the seven clips of CASES (each
stage fed with the oracle's previous stage rounded to fp32; "e2e" is the whole chain), and for the four sampled clips of the
B = 256, L = 65280 batch. Every input carries a noise floor: a bin at fp32 rounding level has an arbitrary angle, and a pure tone
would make the fp32 and fp64 phase sums diverge legitimately.

Measured on an MI355X (docs/experiments.md, "Waveform augmentations on the GPU"; the tests print every figure), worst clip per length:
STFT 7.8e-8 .. 1.1e-7, vocoder 3.8e-7 .. 7.4e-7 (synthetic spectra 3.8e-6), inverse STFT 1.9e-7 .. 2.1e-7, finish 5.4e-7 .. 6.5e-7, end
to end 5.9e-7 .. 6.6e-7 at L <= 3000, 1.6e-6 at 8192, 3.3e-6 at 8229, 2.5e-6 on the sampled clips of the training batch; rate 1 returns the
input within 3.4e-7."""
import functools
import math

import numpy as np
import pytest
import torch

import augment_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875,
       "arch": "grafp", "gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5}
LENGTHS = (1025, 1500, 3000, 8192, 8229)              # below one frame, L % hop zero and non-zero, odd lengths
# (mode, rate) per clip: rates {0.7, 1.0, 1.2345, 1.5}, semitones {-3, 0.5, 3}; B = 5 with mixed modes, and B = 1
CASES = {"b5": [(0, 0.7), (1, A.pitch_rate(-3)), (0, 1.2345), (1, A.pitch_rate(3)), (0, 1.5)],
         "b1_stretch": [(0, 1.0)], "b1_pitch": [(1, A.pitch_rate(0.5))]}
GAINS = (1.7, 0.4, 1.0, 2.9, 0.33)
HEADROOM = 30.0
# fp32 oracle vs fp64 oracle, CPU: worst clip of CASES per length and stage
FLOOR = {
    1025: {"stft": 7.79e-08, "vocoder": 4.46e-07, "istft": 2.12e-07, "finish": 2.26e-07, "e2e": 3.41e-07},
    1500: {"stft": 8.95e-08, "vocoder": 3.55e-07, "istft": 1.59e-07, "finish": 2.10e-07, "e2e": 3.41e-07},
    3000: {"stft": 8.38e-08, "vocoder": 3.41e-07, "istft": 1.83e-07, "finish": 3.31e-07, "e2e": 4.20e-07},
    8192: {"stft": 8.86e-08, "vocoder": 5.43e-07, "istft": 2.01e-07, "finish": 2.47e-07, "e2e": 1.99e-06},
    8229: {"stft": 9.21e-08, "vocoder": 7.43e-07, "istft": 2.17e-07, "finish": 2.59e-07, "e2e": 4.78e-06},
}
L_TRAIN, B_TRAIN = 65280, 256
TRAIN_CLIPS = {3: (0, 0.7), 77: (1, A.pitch_rate(3)), 130: (1, A.pitch_rate(-3)), 255: (0, 1.5)}      # clip -> (mode, rate)
FLOOR_TRAIN = 3.01e-06                                # worst of the four sampled clips (3.0e-6, 1.8e-6, 1.9e-6, 2.4e-6)


def wave_n(n, seed):
    """tests/test_frontend_batch_gpu.py::wave_n: tones + 0.05 noise + edge taper"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / CFG["fs"]
    x = 0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.1 * torch.sin(2 * math.pi * 3100.0 * t * (1 + 0.05 * t))
    x = x + 0.05 * torch.randn(n, generator=g)
    return (x * torch.hann_window(n, periodic=False).clamp_min(0.05)).float()


def noise_n(n, seed):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def counters(reset=False):
    from neuralsampleid_amd import _lib
    return _lib.launch_counters(reset=reset)


def module(**kw):
    from neuralsampleid_amd.modules.transformations import GPUWaveAugment
    return GPUWaveAugment(CFG, **kw)


def params_of(case, dev=DEV):
    from neuralsampleid_amd.modules.transformations import WaveAugmentParams
    B = len(case)
    return WaveAugmentParams(torch.tensor(GAINS[:B], dtype=torch.float32, device=dev),
                             torch.tensor([m for m, _ in case], dtype=torch.int32, device=dev),
                             torch.tensor([float(r) for _, r in case], dtype=torch.float32, device=dev))


@functools.lru_cache(maxsize=None)
def inputs(L, B):
    """x_i: the remaining stem (noise), x_j: the sample stems (tones + noise), (B, L) float32 on the host"""
    return (torch.stack([noise_n(L, 50 + b) for b in range(B)]), torch.stack([wave_n(L, 10 + b) for b in range(B)]))


def chain(x_i, x_j, gain, mode, rate, dt):
    """the four oracle stages of one clip in `dt`, each fed with the fp64 chain's previous stage rounded to fp32"""
    r, L = A.rate64(rate), len(x_i)
    D = A.stft(A.mix(x_i, x_j, np.float32(gain), np.float64), np.float64)
    D32 = D.astype(np.complex64)
    S = A.vocoder(D32.astype(np.complex128), r, np.float64)
    S32 = S.astype(np.complex64)
    n_s = A.stretched_len(L, r)
    s = A.istft(S32.astype(np.complex128), n_s, np.float64)
    s32 = s.astype(np.float32)
    o = A.finish(s32.astype(np.float64), r, mode, L, np.float64)
    ref = {"D32": D32, "S32": S32, "s32": s32, "stft": D, "vocoder": S, "istft": s, "finish": o}
    if dt == np.float32:
        ref = dict(ref, stft=A.stft(A.mix(x_i, x_j, np.float32(gain), np.float32), np.float32), vocoder=A.vocoder(D32, r, np.float32),
                   istft=A.istft(S32, n_s, np.float32), finish=A.finish(s32, r, mode, L, np.float32))
    return ref


@functools.lru_cache(maxsize=None)
def reference(L, name):
    """per clip of the case: the fp64 stage chain and the fp64 end-to-end result; computed once and shared"""
    case = CASES[name]
    x_i, x_j = inputs(L, len(case))
    out = []
    for b, (mode, rate) in enumerate(case):
        xi, xj = x_i[b].numpy(), x_j[b].numpy()
        ref = chain(xi, xj, GAINS[b], mode, rate, np.float64)
        ref["e2e"] = A.augment(xi, xj, np.float32(GAINS[b]), mode, rate, np.float64)
        out.append(ref)
    return out


def check(what, L, stage, got, want, bound=None):
    bound = HEADROOM * FLOOR[L][stage] if bound is None else bound
    errs = [A.rel(g, w) for g, w in zip(got, want)]
    print(f"{what} L={L}: worst {max(errs):.3e} (per clip {' '.join(f'{e:.1e}' for e in errs)}), bound {bound:.3e}")
    assert all(np.isfinite(np.asarray(g)).all() for g in got)
    assert max(errs) <= bound


def c64(t):
    """(.., 2) float32 device tensor -> complex64 numpy"""
    return torch.view_as_complex(t.contiguous()).cpu().numpy()


def tables():
    from neuralsampleid_amd.modules import transformations as T
    from neuralsampleid_amd import ops
    win = torch.hann_window(ops.AUG_N_FFT, periodic=True, dtype=torch.float64).to(torch.float32).to(DEV)
    return win, T.aug_twiddles().to(DEV), torch.from_numpy(T.aug_filter_table().astype(np.float32)).to(DEV)


STAGE_ARGS = [(L, name) for L in LENGTHS for name in CASES]


@pytest.mark.parametrize("L,name", STAGE_ARGS)
def test_stft_stage(L, name):
    from neuralsampleid_amd import ops
    case, ref = CASES[name], reference(L, name)
    x_i, x_j = inputs(L, len(case))
    p, (win, tw, _) = params_of(case), tables()
    spec = c64(ops.aug_stft(x_i.to(DEV), x_j.to(DEV), p.gain, win, tw))
    assert spec.shape == (len(case), 1 + L // 512, 1025)
    check(f"stft {name}", L, "stft", list(spec), [r["stft"] for r in ref])


def _pad_frames(a, T):
    out = np.zeros((T, 1025), np.complex64)
    out[:len(a)] = a
    return out


@pytest.mark.parametrize("L,name", STAGE_ARGS)
def test_vocoder_stage(L, name):
    from neuralsampleid_amd import ops
    case, ref, m = CASES[name], reference(L, name), module()
    p, B = params_of(case), len(case)
    D = torch.view_as_real(torch.from_numpy(np.stack([r["D32"] for r in ref]))).contiguous().to(DEV)
    out = c64(ops.aug_vocoder(D, B, L, p.rate, m.rate_lo, m.rate_hi))
    assert out.shape == (B, m.extents(L)[1], 1025)
    check(f"vocoder {name}", L, "vocoder", [out[b, :len(r["vocoder"])] for b, r in enumerate(ref)], [r["vocoder"] for r in ref])


def test_vocoder_stage_on_synthetic_spectra():
    """magnitudes bounded away from zero (0.5 .. 1.5), uniform phases: every angle is well conditioned, so the bound is the fp32
    floor of this input alone (measured on the CPU: see SYNTH_FLOOR)"""
    from neuralsampleid_amd import ops
    L, m = 8229, module()
    D32, rates = synthetic_spectra(L)
    want = [A.vocoder(D32[b].astype(np.complex128), A.rate64(r), np.float64) for b, r in enumerate(rates)]
    D = torch.view_as_real(torch.from_numpy(D32)).contiguous().to(DEV)
    out = c64(ops.aug_vocoder(D, len(rates), L, torch.tensor(rates, dtype=torch.float32, device=DEV), m.rate_lo, m.rate_hi))
    check("vocoder synthetic", L, "vocoder", [out[b, :len(w)] for b, w in enumerate(want)], want, bound=HEADROOM * SYNTH_FLOOR)


SYNTH_FLOOR = 3.78e-06


def synthetic_spectra(L):
    g = np.random.default_rng(5)
    T = A.frames_in(L)
    rates = [np.float32(0.7), np.float32(1.0), np.float32(1.2345), np.float32(1.5), A.pitch_rate(0.5)]
    mag = 0.5 + g.random((len(rates), T, 1025))
    ph = 2 * np.pi * g.random((len(rates), T, 1025))
    return (mag * np.exp(1j * ph)).astype(np.complex64), rates


@pytest.mark.parametrize("L,name", STAGE_ARGS)
def test_istft_stage(L, name):
    from neuralsampleid_amd import ops
    case, ref, m = CASES[name], reference(L, name), module()
    p, B = params_of(case), len(case)
    T_max = m.extents(L)[1]
    S = torch.view_as_real(torch.from_numpy(np.stack([_pad_frames(r["S32"], T_max) for r in ref]))).contiguous().to(DEV)
    win, tw, _ = tables()
    wave = ops.aug_istft(S, B, L, p.rate, m.rate_lo, m.rate_hi, win, tw).cpu().numpy()
    assert wave.shape == (B, m.extents(L)[2])
    check(f"istft {name}", L, "istft", [wave[b, :len(r["istft"])] for b, r in enumerate(ref)], [r["istft"] for r in ref])


@pytest.mark.parametrize("L,name", STAGE_ARGS)
def test_finish_stage(L, name):
    from neuralsampleid_amd import ops
    case, ref, m = CASES[name], reference(L, name), module()
    p, B = params_of(case), len(case)
    S_max = m.extents(L)[2]
    s = np.full((B, S_max), np.nan, np.float32)                             # past n_s: never read
    for b, r in enumerate(ref):
        s[b, :len(r["s32"])] = r["s32"]
    out = ops.aug_finish(torch.from_numpy(s).to(DEV), B, L, p.mode, p.rate, m.rate_lo, m.rate_hi, tables()[2]).cpu().numpy()
    assert out.shape == (B, L)
    check(f"finish {name}", L, "finish", list(out), [r["finish"] for r in ref])


@pytest.mark.parametrize("L,name", STAGE_ARGS)
def test_forward_end_to_end(L, name):
    case, ref, m = CASES[name], reference(L, name), module()
    x_i, x_j = inputs(L, len(case))
    xj = x_j.to(DEV)
    before = counters()
    out, same = m(x_i.to(DEV), xj, params_of(case))
    after = counters()
    assert same is xj and out.shape == (len(case), L) and out.dtype == torch.float32
    assert all(after[k] - before[k] == 1 for k in ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish"))
    check(f"forward {name}", L, "e2e", list(out.cpu().numpy()), [r["e2e"] for r in ref])


@functools.lru_cache(maxsize=None)
def train_batch():
    g = torch.Generator().manual_seed(1)
    x_i = 0.1 * torch.randn(B_TRAIN, L_TRAIN, generator=g)
    x_j = 0.1 * torch.randn(B_TRAIN, L_TRAIN, generator=g)
    for b in TRAIN_CLIPS:
        x_i[b], x_j[b] = noise_n(L_TRAIN, 300 + b), wave_n(L_TRAIN, 200 + b)
    p = module().draw(B_TRAIN, generator=torch.Generator().manual_seed(2), device="cpu")
    mode, rate = p.mode.clone(), p.rate.clone()
    for b, (mo, r) in TRAIN_CLIPS.items():
        mode[b], rate[b] = mo, float(r)
    return x_i, x_j, p.gain, mode, rate


def test_training_batch():
    """B = 256 clips of 4.08 s with drawn parameters: four sampled clips (both modes, both ends of the rate range) against fp64,
    all 256 finite; four launches per chunk of 64 clips"""
    from neuralsampleid_amd.modules.transformations import WaveAugmentParams
    x_i, x_j, gain, mode, rate = train_batch()
    m = module()
    before = counters()
    out, _ = m(x_i.to(DEV), x_j.to(DEV), WaveAugmentParams(gain.to(DEV), mode.to(DEV), rate.to(DEV)))
    after = counters()
    assert all(after[k] - before[k] == 4 for k in ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish"))
    out = out.cpu()
    assert out.shape == (B_TRAIN, L_TRAIN) and bool(torch.isfinite(out).all())
    assert float(out.abs().amax(1).min()) > 0.01                              # no clip came back empty
    want = [A.augment(x_i[b].numpy(), x_j[b].numpy(), gain[b].numpy(), int(mode[b]), rate[b].numpy()) for b in TRAIN_CLIPS]
    check("training batch", L_TRAIN, "e2e", [out[b].numpy() for b in TRAIN_CLIPS], want, bound=HEADROOM * FLOOR_TRAIN)


# ---- exact properties
def test_no_transform_returns_the_samples():
    """max_transforms_1 = max_transforms_2 = 0 and x_i = 0: gain 1, rate 1, and the chain is the identity within the e2e bound"""
    m = module(max_transforms_1=0, max_transforms_2=0)
    for L in (1500, 8229):
        _, x_j = inputs(L, 5)
        out, _ = m(torch.zeros(5, L, device=DEV), x_j.to(DEV), params_of(CASES["b5"]))      # the given draw is overridden
        check("identity", L, "e2e", list(out.cpu().numpy()), list(x_j.numpy().astype(np.float64)))
    assert bool((m.draw(4).rate == 1).all())


def test_zero_input_gives_zero_output():
    m = module()
    z = torch.zeros(5, 3000, device=DEV)
    out, _ = m(z, z, params_of(CASES["b5"]))
    assert bool(torch.isfinite(out).all()) and bool((out == 0).all()) and not bool(torch.signbit(out).any())


def test_tail_past_the_stretched_length_is_exactly_zero():
    L, m = 8229, module()
    x_i, x_j = inputs(L, 5)
    out, _ = m(x_i.to(DEV), x_j.to(DEV), params_of(CASES["b5"]))
    out = out.cpu()
    for b, (mode, rate) in enumerate(CASES["b5"]):
        r = A.rate64(rate)
        n_s = A.stretched_len(L, r)
        end = min(L, n_s if mode == 0 else A.resampled_len(n_s, r))
        assert bool((out[b, end:] == 0).all()) and float(out[b, max(0, end - 256):end].abs().max()) > 0
    assert A.stretched_len(L, 1.5) < L                                        # the rate 1.5 clip does have a tail


def test_a_clip_does_not_depend_on_its_batch():
    L, m = 3000, module()
    x_i, x_j = inputs(L, 5)
    xi, xj, p = x_i.to(DEV), x_j.to(DEV), params_of(CASES["b5"])
    a = m(xi, xj, p)[0].clone()
    assert torch.equal(a, m(xi, xj, p)[0])                                    # between two runs
    from neuralsampleid_amd.modules.transformations import WaveAugmentParams
    for b in range(5):
        alone = m(xi[b:b + 1].clone(), xj[b:b + 1].clone(), WaveAugmentParams(p.gain[b:b + 1].clone(), p.mode[b:b + 1].clone(),
                                                                              p.rate[b:b + 1].clone()))[0]
        assert torch.equal(alone[0], a[b])


def test_strided_views_equal_contiguous_input():
    L, m = 3000, module()
    x_i, x_j = inputs(L, 5)
    p = params_of(CASES["b5"])
    want = m(x_i.to(DEV), x_j.to(DEV), p)[0]
    views = []
    for x in (x_i, x_j):
        big = torch.full((5 * (L + 107) + 3,), float("nan"), device=DEV)
        v = big[3:].view(5, L + 107)[:, :L]                                   # odd first offset, NaN in the gaps
        v.copy_(x)
        assert v.stride(0) == L + 107 and v.storage_offset() == 3
        views.append(v)
    assert torch.equal(m(views[0], views[1], p)[0], want)


def test_parameters_outside_the_bounds_are_clamped():
    """rates below / above the declared bounds and NaN are ordinary inputs to the clamp: the result is the clamped clip's"""
    from neuralsampleid_amd.modules.transformations import WaveAugmentParams
    L, m = 3000, module()
    x_i, x_j = inputs(L, 5)
    xi, xj = x_i.to(DEV), x_j.to(DEV)
    gain = torch.tensor(GAINS, device=DEV)
    mode = torch.tensor([0, 1, 0, 1, 7], dtype=torch.int32, device=DEV)       # a mode other than 1 is 0
    odd = torch.tensor([0.01, 1e9, float("nan"), float("nan"), -3.0], device=DEV)
    lo, hi = m.rate_lo, m.rate_hi
    clamped = torch.tensor([lo, hi, lo, lo, lo], device=DEV)
    got = m(xi, xj, WaveAugmentParams(gain, mode, odd))[0]
    want = m(xi, xj, WaveAugmentParams(gain, torch.tensor([0, 1, 0, 1, 0], dtype=torch.int32, device=DEV), clamped))[0]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_forward_is_capturable():
    """one stream, torch.cuda.graph; replay after inputs and the three parameter tensors changed in place = eager on the new contents"""
    from neuralsampleid_amd.modules.transformations import WaveAugmentParams
    L, m = 3000, module()
    x_i, x_j = inputs(L, 5)
    xi, xj = x_i.to(DEV).clone(), x_j.to(DEV).clone()
    p = params_of(CASES["b5"])
    p = WaveAugmentParams(p.gain.clone(), p.mode.clone(), p.rate.clone())
    m(xi, xj, p)                                                              # tables and workspaces exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    counters(reset=True)
    with torch.cuda.graph(graph):
        out, _ = m(xi, xj, p)
    cap = counters()
    assert all(cap[k] == 1 for k in ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish"))
    assert sum(cap.values()) == 4                                             # none of the GEMM path's, nothing else
    xi.copy_(x_j.to(DEV) * 0.5)
    xj.copy_(x_i.to(DEV) + 0.2 * x_j.to(DEV))
    p.gain.copy_(torch.tensor([0.5, 2.0, 1.1, 0.9, 3.0], device=DEV))
    p.mode.copy_(torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32, device=DEV))
    p.rate.copy_(torch.tensor([0.9, 1.4, 1.1, 0.75, 0.85], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = m(xi, xj, p)[0]
    assert torch.equal(out, eager)


def test_host_checks_launch_nothing():
    from neuralsampleid_amd import _lib, ops
    L, B = 3000, 2
    win, tw, tab = tables()
    m = module()
    T_in, T_max, S_max = m.extents(L)
    x = torch.zeros(B, L, device=DEV)
    gain, rate, mode = torch.ones(B, device=DEV), torch.ones(B, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    spec = torch.zeros(B, T_in, 1025, 2, device=DEV)
    voc = torch.zeros(B, T_max, 1025, 2, device=DEV)
    wave = torch.zeros(B, S_max, device=DEV)
    out = torch.zeros(B, L, device=DEV)
    P, lib, s = ops._p, _lib.lib, ops._stream()
    lo, hi = m.rate_lo, m.rate_hi
    counters(reset=True)
    bad = [
        lib.nsid_aug_stft(P(x), L, P(x), L, B, 0, P(gain), P(win), P(tw), P(spec), s),                  # L < 1
        lib.nsid_aug_stft(P(x), L, P(x), L, B, 1 << 30, P(gain), P(win), P(tw), P(spec), s),            # L >= 2^30
        lib.nsid_aug_stft(P(x), L - 1, P(x), L, B, L, P(gain), P(win), P(tw), P(spec), s),              # stride shorter than a row
        lib.nsid_aug_stft(P(x), L, P(x), L, B, L, P(gain), P(win), P(tw) + 4, P(spec), s),              # misaligned twiddles
        lib.nsid_aug_stft(P(x), L, P(x), L, B, L, None, P(win), P(tw), P(spec), s),                     # null
        lib.nsid_aug_vocoder(P(spec), B, L, P(rate), 0.0, hi, P(voc), T_max, s),                        # rate_lo <= 0
        lib.nsid_aug_vocoder(P(spec), B, L, P(rate), 1.6, hi, P(voc), T_max, s),                        # rate_lo > rate_hi
        lib.nsid_aug_vocoder(P(spec), B, L, P(rate), lo, hi, P(voc), T_max - 1, s),                     # workspace too short
        lib.nsid_aug_istft(P(voc), T_max, B, L, P(rate), lo, hi, P(win), P(tw), P(wave), S_max - 1, s),
        lib.nsid_aug_istft(P(voc), T_max, B, L, P(rate), -1.0, hi, P(win), P(tw), P(wave), S_max, s),
        lib.nsid_aug_istft(P(voc), T_max, B, L, P(rate), lo, hi, P(win), P(tw) + 4, P(wave), S_max, s),
        lib.nsid_aug_finish(P(wave), S_max, B, L, P(mode), P(rate), lo, hi, P(tab), P(out), L - 1, s),
        lib.nsid_aug_finish(P(wave), S_max - 1, B, L, P(mode), P(rate), lo, hi, P(tab), P(out), L, s),
        lib.nsid_aug_finish(P(wave), S_max, B, L, P(mode), P(rate), float("nan"), hi, P(tab), P(out), L, s),
        lib.nsid_aug_finish(P(wave), S_max, B, L, None, P(rate), lo, hi, P(tab), P(out), L, s),
    ]
    assert bad == [-1] * len(bad)
    assert sum(counters().values()) == 0
    torch.cuda.synchronize()
