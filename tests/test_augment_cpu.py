"""CPU: the shells around the waveform augmentations (csrc/augment.hip, nsid_aug_*; modules/transformations.GPUWaveAugment) -- the
bindings and counters, the host-side tables, the parameter draw, the extent arithmetic -- and the semantics of the oracle
restatement itself (tests/augment_oracle.py) in fp64. No GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

import augment_oracle as A

CFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875,
       "arch": "grafp", "gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5}
ENTRIES = {"nsid_aug_stft": "plplilpppps", "nsid_aug_vocoder": "pilpffpls", "nsid_aug_istft": "plilpffpppls",
           "nsid_aug_finish": "plilppffppls"}


def module(**kw):
    from neuralsampleid_amd.modules.transformations import GPUWaveAugment
    return GPUWaveAugment(CFG, **kw)


def test_entry_points_are_bound_and_counted():
    from neuralsampleid_amd import _lib
    keys = ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish")
    for name, sig in ENTRIES.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(_lib.lib, name)
    before = _lib.launch_counters()
    assert all(k in before for k in keys)
    assert not hasattr(_lib.lib, "nsid_aug") and not hasattr(_lib.lib, "nsid_aug_all")      # stages only, no all-in-one entry
    # null arguments are refused on the host before any launch: NSID_EINVAL = -1, and nothing is counted
    L = 65280
    assert _lib.lib.nsid_aug_stft(None, L, None, L, 1, L, None, None, None, None, None) == -1
    assert _lib.lib.nsid_aug_vocoder(None, 1, L, None, 0.7, 1.5, None, 183, None) == -1
    assert _lib.lib.nsid_aug_istft(None, 183, 1, L, None, 0.7, 1.5, None, None, None, 93258, None) == -1
    assert _lib.lib.nsid_aug_finish(None, 93258, 1, L, None, None, 0.7, 1.5, None, None, L, None) == -1
    after = _lib.launch_counters()
    assert all(after[k] == before[k] for k in keys)


def _ulp(want):
    return np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 23), 1e-16)


def test_tables_are_within_one_ulp_of_fp64():
    from neuralsampleid_amd.modules import transformations as T
    tw = T.aug_twiddles()
    assert tw.shape == (2048, 2) and tw.dtype == torch.float32 and tw.is_contiguous()
    j = np.arange(2048, dtype=np.float64)
    want = np.stack((np.cos(-2 * np.pi * j / 2048), np.sin(-2 * np.pi * j / 2048)), 1)
    assert bool((np.abs(tw.double().numpy() - want) <= _ulp(want)).all())
    assert float(tw[0, 0]) == 1.0 and float(tw[0, 1]) == 0.0 and float(tw[512, 1]) == -1.0 and float(tw[1024, 0]) == -1.0
    tab = T.aug_filter_table()
    n = 64 * 512
    assert tab.dtype == np.float64 and tab.shape == (n + 1,)
    # an independent fp64 evaluation: Kaiser window through I0's series, sinc through sin
    u = np.linspace(0, 64, n + 1)
    i0 = lambda x: sum((x / 2) ** (2 * k) / math.factorial(k) ** 2 for k in range(60))
    kais = i0(T.AUG_BETA * np.sqrt(np.maximum(0.0, 1 - (u / 64) ** 2))) / i0(T.AUG_BETA)
    arg = np.pi * T.AUG_ROLLOFF * u
    sinc = np.where(u == 0, 1.0, np.sin(arg) / np.where(u == 0, 1.0, arg))
    want = kais * T.AUG_ROLLOFF * sinc
    # 1 ulp of fp32 at the value's magnitude, plus fp64 evaluation noise of the two routes at the scale of the table's peak
    assert bool((np.abs(tab.astype(np.float32).astype(np.float64) - want) <= _ulp(want) + 1e-13).all())
    assert tab[0] == T.AUG_ROLLOFF and abs(tab[-1]) < 1e-7
    assert np.array_equal(tab, A.TABLE)                                     # the oracle reads the same definition


def test_draw_is_reproducible_and_in_range():
    m = module()
    g = torch.Generator().manual_seed(7)
    p = m.draw(512, generator=g, device="cpu")
    q = m.draw(512, generator=torch.Generator().manual_seed(7), device="cpu")
    for a, b in zip(p[:3], q[:3]):
        assert torch.equal(a, b)
    torch.manual_seed(11)
    r1 = m.draw(64, device="cpu")
    torch.manual_seed(11)
    r2 = m.draw(64, device="cpu")
    assert torch.equal(r1.rate, r2.rate) and torch.equal(r1.mode, r2.mode) and torch.equal(r1.gain, r2.gain)
    assert p.gain.dtype == torch.float32 and p.mode.dtype == torch.int32 and p.rate.dtype == torch.float32
    assert p.gain.shape == p.mode.shape == p.rate.shape == (512,)
    db = 20 * torch.log10(p.gain.double())
    assert float(db.abs().max()) <= 10 + 1e-5 and float(db.max()) > 5 and float(db.min()) < -5
    assert set(p.mode.tolist()) == {0, 1} and 150 < int(p.mode.sum()) < 362
    st, pi = p.mode == 0, p.mode == 1
    assert float(p.rate[st].min()) >= np.float32(0.7) and float(p.rate[st].max()) <= np.float32(1.5)
    n = p.semitones[pi]
    assert float(n.abs().max()) <= 3 and bool(torch.isnan(p.semitones[st]).all())
    want = torch.pow(2.0, -n / 12.0).to(torch.float32)                       # fp64 first, one rounding
    assert torch.equal(p.rate[pi], want)
    assert float(p.rate.min()) >= m.rate_lo and float(p.rate.max()) <= m.rate_hi
    off = module(max_transforms_1=0, max_transforms_2=0).draw(16, device="cpu")
    assert bool((off.gain == 1).all()) and bool((off.rate == 1).all()) and bool((off.mode == 0).all())


def test_host_extents_equal_the_oracles_lengths():
    from neuralsampleid_amd import ops
    m = module()
    assert m.rate_lo == float(np.float32(0.7)) and m.rate_hi == float(np.float32(1.5))
    rates = np.concatenate([np.linspace(0.7, 1.5, 500), 2.0 ** (-np.linspace(-3, 3, 500) / 12)]).astype(np.float32)
    for L in (1025, 8229, 65280):
        T_in, T_max, S_max = m.extents(L)
        assert T_in == A.frames_in(L) == ops.aug_frames_in(L)
        assert T_max == A.frames_out(T_in, m.rate_lo) and S_max == A.stretched_len(L, m.rate_lo)
        for rate in rates:
            r = A.rate64(rate)
            T_out, n_s = A.frames_out(T_in, r), A.stretched_len(L, r)
            assert T_out <= T_max and n_s <= S_max
            # the arithmetic the kernels do in fp64: ceil(T_in / r), rint(L / r), ceil(n_s r)
            assert T_out == int(np.ceil(np.float64(T_in) / np.float64(r))) == len(np.arange(0, T_in, r))
            assert n_s == int(np.rint(np.float64(L) / np.float64(r)))
            assert A.resampled_len(n_s, r) == int(np.ceil(np.float64(n_s) * np.float64(r))) >= L
    assert m.workspace_bytes(256, 65280) == 64 * ((128 + 183) * 1025 * 8 + 93257 * 4)
    assert m.extents(65280) == (128, 183, 93257)


def test_module_shell():
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID, GPUWaveAugment
    sig = inspect.signature(GPUWaveAugment.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("cfg", inspect.Parameter.empty), ("max_transforms_1", 1), ("max_transforms_2", 1)]
    assert list(inspect.signature(GPUWaveAugment.forward).parameters) == ["self", "x_i", "x_j", "params"]
    m = module()
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 3000), torch.zeros(2, 3000))                        # host tensors: refused, not computed elsewhere
    with pytest.raises(NotImplementedError):
        GPUWaveAugment(dict(CFG, arch="resnet-ibn"))
    # the spectrogram module is unchanged: same signature, cpu=True still raises and now names the device module too
    sig = inspect.signature(GPUTransformSampleID.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("cfg", inspect.Parameter.empty), ("ir_dir", None), ("train", True), ("cpu", False),
        ("max_transforms_1", 1), ("max_transforms_2", 1)]
    with pytest.raises(NotImplementedError, match="audiomentations"):
        GPUTransformSampleID(CFG, cpu=True)
    with pytest.raises(NotImplementedError, match="GPUWaveAugment"):
        GPUTransformSampleID(CFG, cpu=True)


# ---- the oracle's own semantics, fp64
def tone(L, f=1000.0, noise=1e-3):
    t = np.arange(L) / 16000
    return 0.5 * np.sin(2 * np.pi * f * t) + noise * np.random.default_rng(0).standard_normal(L)


def peak_hz(x):
    X = np.abs(np.fft.rfft(x * np.hanning(len(x))))
    return X.argmax() * 16000 / len(x)


def test_oracle_rate_one_is_the_identity():
    for L in (1025, 3000, 8229):
        y = tone(L, noise=0.05)
        assert A.rel(A.time_stretch(y, 1.0), y) < 1e-12
        assert A.rel(A.augment(np.zeros(L), y, 1.0, 0, 1.0), y) < 1e-12


def test_oracle_stretch_keeps_the_frequency():
    L = 32768
    y = tone(L)
    for rate in (0.7, 1.5):
        s = A.time_stretch(y, rate)
        assert len(s) == int(np.rint(L / float(np.float32(rate))))
        assert abs(peak_hz(s) - 1000.0) <= 16000 / len(s)                    # one bin of the analysis of the stretched clip


def test_oracle_pitch_shift_moves_the_tone():
    L = 32768
    y = tone(L)
    for n in (3.0, -3.0):
        p = A.pitch_shift(y, n)
        assert len(p) == L
        assert abs(peak_hz(p) - 1000.0 * 2 ** (n / 12)) <= 16000 / L         # measured: 1189.0 and 840.8 Hz
