"""CPU: the oracle restatement of the baseline's waveform effects (tests/baseline_augment_oracle.py) on hand cases and against
scipy, the in-package Butterworth design (modules/transformations.butter_bandpass_sos) against scipy.signal.butter, and
GPUBaselineWaveAugment.draw(): reproducible, every value inside its configured range, the mode frequencies.

The Butterworth comparison filters a noise clip through both section tables with the oracle's cascade in np.longdouble, so that what is
left is the difference of the two designs' coefficients (both fp64, a few ulp apart, pairing and section order may differ) and not
the rounding of a recursion. Bound 1e-8 relative to the output's peak: a coefficient error d ~ 1e-15 moves a pole's angle by
d / (2 sin theta) and its radius by d / 2; the response near the pass band changes by that over the pole's distance 1 - r from the
unit circle. The worst case here, the 1 % band at 50 Hz (theta = 0.0142, 1 - r = 7e-5), gives 4e-14 / 7e-5 = 5e-10 per section."""
import numpy as np
import pytest
import torch

import baseline_augment_oracle as O

CFG = {"arch": "resnet-ibn", "fs": 22050, "dur": 5.0, "gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5,
       "DC_threshold": [-30, 0], "DC_ratio": [2, 4, 8, 20], "DC_attack": [0.001, 0.1], "DC_release": [0.05, 1.0]}
FS = 22050.0
# (order, lo, hi): every order, the 1 % band at 50 Hz, a band clamped at 0.9999 Nyquist
DESIGNS = [(2, 300.0, 900.0), (3, 1000.0, 1800.0), (4, 2000.0, 5000.0), (4, 49.75, 50.25), (2, 49.75, 50.25),
           (3, 6000.0, 0.9999 * 0.5 * FS), (4, 8000.0, 0.9999 * 0.5 * FS)]
DESIGN_BOUND = 1e-8


def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def module(**kw):
    from neuralsampleid_amd.modules.transformations import GPUBaselineWaveAugment
    return GPUBaselineWaveAugment(CFG, **kw)


def test_compressor_hand_case():
    y = O.compress(np.array([0.125, 1.0, 0.125, 0.75], np.float32), 0.5, 2.0, 0.0, 0.0)
    assert y.dtype == np.float32 and y.tolist() == [0.125, 0.75, 0.09375, 0.46875]


def test_compressor_returns_input_below_the_threshold_bit_for_bit():
    x = noise(4000, 1)
    x[7] = -0.0
    y = O.compress(x, float(np.abs(x).max()), 4.0, 0.9, 0.99)          # |x| == threshold is not above it
    assert y.tobytes() == x.tobytes()


def test_frame_edits_hand_cases():
    x = np.arange(10, dtype=np.float32)
    got = O.to_length(O.frames(x, 4, [O.OP_DUPLICATE, 0, O.OP_REMOVE]), 10)
    assert got.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    assert O.to_length(O.frames(x, 4, [O.OP_REMOVE] * 3), 10).tolist() == [0] * 10
    both = O.frames(x + 1, 4, [O.OP_SILENCE | O.OP_DUPLICATE, 0, 0])
    assert both.tolist() == [0] * 8 + [5, 6, 7, 8, 9, 10]
    assert O.frames(x, 4, [O.OP_REMOVE | O.OP_DUPLICATE | O.OP_SILENCE, 0, O.OP_DUPLICATE]).tolist() == [4, 5, 6, 7, 8, 9, 8, 9]


def test_eq_oracle_against_sosfilt():
    signal = pytest.importorskip("scipy.signal")
    x = noise(3000, 2)
    bands = [(signal.butter(o, [lo, hi], "bandpass", fs=FS, output="sos"), g) for (o, lo, hi), g in
             zip(DESIGNS[:3], (-6.0, 3.0, -20.0))]
    want = x.astype(np.float64)
    for sos, g in bands:
        assert np.all(sos[:, 3] == 1.0)
        want = signal.sosfilt(sos, want) * 10.0 ** (g / 20.0)
    got = O.band_eq(x, [(np.delete(sos, 3, 1), g) for sos, g in bands], np.float64)
    # one arithmetic in one order; scipy's compiled loop may contract a product into its addition
    assert O.rel(got, want) <= 1e-12


@pytest.mark.parametrize("order,lo,hi", DESIGNS)
def test_butterworth_design_against_scipy(order, lo, hi):
    signal = pytest.importorskip("scipy.signal")
    from neuralsampleid_amd.modules.transformations import butter_bandpass_sos
    mine = butter_bandpass_sos(order, lo, hi, FS)
    ref = signal.butter(order, [lo, hi], "bandpass", fs=FS, output="sos")
    assert mine.shape == (order, 5) and ref.shape == (order, 6)
    x = noise(6000, 3)
    one = np.ones((order, 1))
    got = O.cascade(x, np.concatenate([mine, one], 1), np.longdouble)
    want = O.cascade(x, np.concatenate([np.delete(ref, 3, 1), one], 1), np.longdouble)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"order {order} [{lo}, {hi}] Hz: {err:.2e}")
    assert np.isfinite(np.asarray(got, np.float64)).all() and float(np.abs(want).max()) > 0
    assert err <= DESIGN_BOUND


def test_construction_draws_the_bands_once():
    a, b = module(generator=torch.Generator().manual_seed(4)), module(generator=torch.Generator().manual_seed(4))
    assert a.num_bands == b.num_bands and a.band_gains_db == b.band_gains_db
    assert 1 <= a.num_bands <= 8 and len(a.band_gains_db) == a.num_bands and all(-20.0 <= g <= 10.0 for g in a.band_gains_db)
    seen = {module(generator=torch.Generator().manual_seed(s)).num_bands for s in range(60)}
    assert seen == set(range(1, 9))


def test_draw_is_reproducible_and_inside_its_ranges():
    m = module(generator=torch.Generator().manual_seed(5))
    B, L = 400, 110250
    p = m.draw(B, generator=torch.Generator().manual_seed(6), device="cpu")
    q = m.draw(B, generator=torch.Generator().manual_seed(6), device="cpu")
    assert all(torch.equal(a, b) for a, b in zip(p, q))
    F = m.frames_max(L)
    assert F == 25
    shapes = {"mode1": (B,), "gain": (B,), "cmp": (B, 4), "sos": (B, 32, 6), "n_sec": (B,), "mode2": (B,), "rate": (B,),
              "frame_size": (B,), "frame_ops": (B, F)}
    assert {k: tuple(getattr(p, k).shape) for k in shapes} == shapes
    assert p.cmp.dtype == p.sos.dtype == torch.float64 and p.gain.dtype == p.rate.dtype == torch.float32
    assert all(getattr(p, k).dtype == torch.int32 for k in ("mode1", "n_sec", "mode2", "frame_size", "frame_ops"))
    m1, m2 = p.mode1.numpy(), p.mode2.numpy()
    assert set(m1) == {0, 1, 2} and set(m2) == {0, 1, 2, 3, 4}
    gain, rate = p.gain.numpy().astype(np.float64), p.rate.numpy().astype(np.float64)
    assert np.all(gain[m1 != 2] == 1.0) and np.all((gain >= 10 ** -0.5 * (1 - 1e-7)) & (gain <= 10 ** 0.5 * (1 + 1e-7)))
    assert np.all(rate[m2 >= 2] == 1.0)
    assert np.all((rate[m2 == 0] >= np.float32(0.7)) & (rate[m2 == 0] <= np.float32(1.5)))
    assert np.all((rate[m2 == 1] >= np.float32(2 ** -0.25)) & (rate[m2 == 1] <= np.float32(2 ** 0.25)))
    thr, ratio, att, rel = p.cmp.numpy().T
    assert np.all((thr >= 10 ** -1.5) & (thr <= 1.0)) and set(ratio) <= {2.0, 4.0, 8.0, 20.0} and len(set(ratio)) == 4
    assert np.all((att >= np.exp(-1 / (FS * 0.001))) & (att <= np.exp(-1 / (FS * 0.1))))
    assert np.all((rel >= np.exp(-1 / (FS * 0.05))) & (rel <= np.exp(-1 / (FS * 1.0))))
    fsz = p.frame_size.numpy()
    assert np.all((fsz >= 4410) & (fsz <= 44100))
    ops = p.frame_ops.numpy()
    for mode, bit in ((2, 1), (3, 2), (4, 4)):
        assert set(np.unique(ops[m2 == mode])) == {0, bit}
    assert not ops[m2 < 2].any()
    n_sec, sos = p.n_sec.numpy(), p.sos.numpy()
    assert np.all(n_sec[m1 != 0] == 0) and np.all((n_sec[m1 == 0] >= 2 * m.num_bands) & (n_sec[m1 == 0] <= 4 * m.num_bands))
    gains = sorted(10.0 ** (g / 20.0) for g in m.band_gains_db)
    for b in np.nonzero(m1 == 0)[0]:
        used, rest = sos[b, :n_sec[b]], sos[b, n_sec[b]:]
        assert np.all(rest == np.array([1.0, 0, 0, 0, 0, 1.0])) and np.isfinite(used).all()
        a1, a2 = used[:, 3], used[:, 4]
        assert np.all((np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2))                # every section is stable
        assert sorted(used[used[:, 5] != 1.0, 5]) == [g for g in gains if g != 1.0]


def test_band_edges_follow_the_stated_definition():
    """centre uniform on the HTK mel scale in [50, 8000] Hz, bandwidth = centre * U(0.01, 1), hi clamped to 0.9999 Nyquist"""
    from neuralsampleid_amd.modules import transformations as T
    assert abs(float(T.mel_to_hz(T.hz_to_mel(440.0))) - 440.0) < 1e-9 and abs(float(T.hz_to_mel(1000.0)) - 1000.0) < 0.05
    m = module(generator=torch.Generator().manual_seed(5))
    a = m.band_sections(8000.0, 1.0, 4)                                           # hi = 12 000 Hz is past Nyquist
    b = T.butter_bandpass_sos(4, 4000.0, 0.9999 * 0.5 * FS, FS)
    assert np.array_equal(a, b)


def test_mode_frequencies():
    m = module(generator=torch.Generator().manual_seed(7))
    N = 20000
    m1, m2 = [], []
    for k in range(4):                                                            # 4 x 5 000 clips: the section design stays cheap
        m_k = module(generator=torch.Generator().manual_seed(7))
        m_k.num_bands, m_k.band_gains_db = 1, [0.0]
        p = m_k.draw(N // 4, generator=torch.Generator().manual_seed(100 + k), device="cpu", L=4410)
        m1.append(p.mode1.numpy())
        m2.append(p.mode2.numpy())
    m1, m2 = np.concatenate(m1), np.concatenate(m2)
    for modes, n_opt in ((m1, 3), (m2, 5)):
        q = 1.0 / n_opt
        sigma = np.sqrt(q * (1 - q) / N)
        freq = np.bincount(modes, minlength=n_opt) / N
        print(n_opt, freq, 4 * sigma)
        assert len(freq) == n_opt and np.all(np.abs(freq - q) <= 4 * sigma)
    assert m.num_bands >= 1


def test_no_transform_draws():
    m = module(max_transforms_1=0, max_transforms_2=0, generator=torch.Generator().manual_seed(8))
    p = m.draw(64, generator=torch.Generator().manual_seed(9), device="cpu")
    assert bool((p.mode1 == 2).all()) and bool((p.gain == 1).all()) and bool((p.mode2 == 0).all()) and bool((p.rate == 1).all())
    assert not bool(p.frame_ops.any()) and bool((p.n_sec == 0).all())


def test_the_grafp_module_keeps_refusing_the_arch():
    from neuralsampleid_amd.modules.transformations import GPUBaselineWaveAugment, GPUWaveAugment
    with pytest.raises(NotImplementedError):
        GPUWaveAugment(CFG)
    with pytest.raises(NotImplementedError):
        GPUBaselineWaveAugment(dict(CFG, arch="grafp"))
