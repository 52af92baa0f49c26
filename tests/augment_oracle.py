"""Test helper (like cqt_oracle.py): the waveform augmentations of DESIGN.md "Waveform augmentations" -- librosa 0.10's
effects.time_stretch / effects.pitch_shift as audiomentations calls them (method "librosa_phase_vocoder"), with the resampler
restated as a tabulated Kaiser-windowed sinc -- in numpy / torch on the CPU, stage by stage, with the arithmetic type of the
values selectable. Written from that description; nothing from the reference tree, no librosa, no scipy.

    r = rate64(rate)                     every index below is fp64 arithmetic on r = float64(float32(rate))
    D = stft(y, dt)                      (T_in, 1025) complex, T_in = 1 + L // 512, center=True with zero padding
    S = vocoder(D, r, dt)                (T_out, 1025), T_out = ceil(T_in / r)
    s = istft(S, n_s, dt)                n_s = rint(L / r) samples
    o = finish(s, r, mode, L, dt)        mode 0: cut / zero-fill to L; mode 1: resample by r (n_out = ceil(n_s r)), then to L
    time_stretch(y, rate, dt), pitch_shift(y, n_steps, dt), augment(x_i, x_j, gain, mode, rate, dt) chain them.

dt = np.float64 is the reference of the tests. dt = np.float32 uses real fp32 FFTs (torch.fft on float32), an fp32 phase sum in the
wrapped form and fp32 dot products: its distance from fp64 is the rounding floor the GPU bounds are multiples of."""
import math

import numpy as np
import torch

N, HOP, BINS = 2048, 512, 1025
ZEROS, PRECISION, ROLLOFF, BETA = 64, 512, 0.9475937167399596, 14.769656459379492


def rate64(rate) -> float:
    return float(np.float32(rate))


def pitch_rate(n_steps) -> np.float32:
    return np.float32(2.0 ** (-float(n_steps) / 12.0))


def frames_in(L):
    return 1 + L // HOP


def frames_out(T_in, r):
    return int(math.ceil(T_in / r))                    # len(np.arange(0, T_in, r))


def stretched_len(L, r):
    return int(round(L / r))                           # Python's round: ties to even


def resampled_len(n_s, r):
    return int(math.ceil(n_s * r))


def window(dt):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(dt)          # periodic Hann


def filter_table():
    n = ZEROS * PRECISION
    return np.kaiser(2 * n + 1, BETA)[n:] * ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, ZEROS, n + 1))


TABLE = filter_table()


def _tt(dt):
    return torch.float64 if dt == np.float64 else torch.float32


def mix(x_i, x_j, gain, dt):
    return (dt(gain) * np.asarray(x_j, dt) + np.asarray(x_i, dt)).astype(dt)


def stft(y, dt):
    yp = torch.from_numpy(np.pad(np.asarray(y, dt), N // 2))
    fr = yp.unfold(0, N, HOP)[:frames_in(len(y))] * torch.from_numpy(window(dt))
    return torch.fft.rfft(fr, dim=1).numpy()                                     # complex64 for fp32 input: a real fp32 FFT


def vocoder(D, r, dt):
    T_in = D.shape[0]
    steps = np.arange(frames_out(T_in, r), dtype=np.float64) * r
    phi = ((np.arange(BINS) % 4) * (np.pi / 2)).astype(dt)                        # 2 pi hop k / n_fft mod 2 pi
    two_pi = dt(2 * np.pi)
    Dp = np.concatenate([D, np.zeros((2, BINS), D.dtype)], 0)
    out = np.zeros((len(steps), BINS), D.dtype)
    acc = np.angle(D[0]).astype(dt)
    for t, s in enumerate(steps):
        c = int(math.floor(s))
        c0, c1 = Dp[min(c, T_in)], Dp[min(c + 1, T_in)]
        a = dt(s - math.floor(s))
        mag = (dt(1) - a) * np.abs(c0).astype(dt) + a * np.abs(c1).astype(dt)
        out[t] = mag * (np.cos(acc) + 1j * np.sin(acc))
        d = np.angle(c1).astype(dt) - np.angle(c0).astype(dt) - phi
        d = d - two_pi * np.round(d / two_pi)
        acc = acc + phi + d
        acc = acc - two_pi * np.round(acc / two_pi)
    return out


def istft(S, length, dt):
    w = window(dt)
    T = S.shape[0]
    fr = torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(S)), n=N, dim=1).numpy().astype(dt) * w
    y, ws = np.zeros(N + HOP * (T - 1), dt), np.zeros(N + HOP * (T - 1), dt)
    for t in range(T):
        y[t * HOP:t * HOP + N] += fr[t]
        ws[t * HOP:t * HOP + N] += w * w
    nz = ws > np.finfo(dt).tiny
    y[nz] /= ws[nz]
    y = y[N // 2:]
    return y[:length] if len(y) >= length else np.pad(y, (0, length - len(y)))


def resample(s, r, n_out, dt):
    """out[m] = c sum_j h(|m / r - j| c) s[j], c = min(1, r), h = TABLE rounded to dt and linearly interpolated, 0 from ZEROS on"""
    c = min(1.0, r)
    tab, s = TABLE.astype(dt), np.asarray(s, dt)
    K = 2 * int(math.ceil(ZEROS / c)) + 3
    out = np.zeros(n_out, dt)
    for m0 in range(0, n_out, 4096):
        pos = np.arange(m0, min(n_out, m0 + 4096), dtype=np.float64) / r
        j = np.floor(pos)[:, None].astype(np.int64) - K // 2 + np.arange(K)[None, :]
        x = np.abs(pos[:, None] - j) * (c * PRECISION)
        ok = (j >= 0) & (j < len(s)) & (x < ZEROS * PRECISION)
        i0 = np.minimum(np.floor(x).astype(np.int64), ZEROS * PRECISION - 1)
        e = (x - i0).astype(dt)
        wgt = tab[i0] + e * (tab[i0 + 1] - tab[i0])
        out[m0:m0 + len(pos)] = dt(c) * np.sum(np.where(ok, wgt * s[np.clip(j, 0, len(s) - 1)], dt(0)), axis=1, dtype=dt)
    return out


def to_length(y, L):
    return y[:L] if len(y) >= L else np.pad(y, (0, L - len(y)))


def finish(s, r, mode, L, dt):
    s = np.asarray(s, dt)
    if mode != 1:
        return to_length(s, L)
    return to_length(resample(s, r, min(resampled_len(len(s), r), L), dt), L)


def stretched(y, r, dt):
    return istft(vocoder(stft(y, dt), r, dt), stretched_len(len(y), r), dt)


def time_stretch(y, rate, dt=np.float64):
    """librosa.effects.time_stretch(y, rate): rint(L / rate) samples"""
    return stretched(y, rate64(rate), dt)


def pitch_shift(y, n_steps, dt=np.float64):
    """librosa.effects.pitch_shift(y, n_steps=n_steps): L samples"""
    r = float(pitch_rate(n_steps))
    return finish(stretched(y, r, dt), r, 1, len(y), dt)


def augment(x_i, x_j, gain, mode, rate, dt=np.float64):
    """one clip of GPUWaveAugment: T2(gain * x_j + x_i) cut / zero-filled to L"""
    r = rate64(rate)
    y = mix(x_i, x_j, gain, dt)
    return finish(stretched(y, r, dt), r, int(mode), len(y), dt)


def rel(a, b):
    """the tests' metric: max |a - b| / max |b| (real or complex)"""
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return float(np.abs(a - b).max() / np.abs(b).max())
